// Host build of the lane bodies of the batched block prover (go-kzg_amd/csrc/sha256_lane.hpp, eth_aggregate.hpp): the resumable SHA-256 and the
// transcript in two halves, the exact source k_eth_transcript_blobs / k_eth_transcript_finish inline, run on a machine without a GPU.
// A plain program with its own main (never loaded into Python; built a second time with the sanitizers):
//     aggregate_prove_emul resume FILE             every line: "<first> <digest>" -- the LEN bytes of FILE hashed with the chain cut after
//                                                  `first` whole blocks and resumed there, for first = 0 .. LEN / 64
//     aggregate_prove_emul transcript N COUNT FILE FILE = COUNT blobs of N x 32 bytes | COUNT commitments of 48 bytes.  Lines:
//                                                  "state <8 words>"   the SHA state after the blob half
//                                                  "prefix <digest>"   that state finished with an empty tail: SHA-256 of the blob half's bytes
//                                                  "halves <r> <z>"    the two lane bodies one after the other (Montgomery limbs, 8 words each)
//                                                  "whole <r> <z>"     eth_transcript_lane on the same bytes
// TEST INFRASTRUCTURE: built by tests/test_compute_aggregate_host.py into tests/host/_build/, never shipped.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "eth_aggregate.hpp"
using namespace kzg;

static std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[4096];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}
static void print_words(const uint32_t *w, int n) { for (int i = 0; i < n; i++) printf("%08x", w[i]); }
static void print_fr(const fr &v) { print_words(v.l, 8); }

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "resume")) {
        const std::vector<uint8_t> m = read_file(argv[2]);   // exactly sized: a read at or past len is the sanitizer's to find
        const uint64_t len = m.size();
        const sha_bytes_src src{m.data()};
        for (uint64_t first = 0; first <= len / 64; first++) {
            uint32_t st[8];
            sha256_init(st);
            sha256_lane_blocks(src, 0, first, st);
            sha256_lane_resume(src, len, first, st);
            printf("%llu ", (unsigned long long)first); print_words(st, 8); printf("\n");
        }
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "transcript")) {
        const uint64_t n = strtoull(argv[2], nullptr, 10), count = strtoull(argv[3], nullptr, 10);
        std::vector<uint8_t> raw = read_file(argv[4]);
        if (raw.size() != count * (n * 32 + 48)) { fprintf(stderr, "file length\n"); return 2; }
        // own 4-byte aligned, exactly sized copies: a read past either part is the sanitizer's to find
        std::vector<uint32_t> blobs(count * n * 8), comms(count * 12);
        if (count) { memcpy(blobs.data(), raw.data(), count * n * 32); memcpy(comms.data(), raw.data() + count * n * 32, count * 48); }
        const uint8_t *b = (const uint8_t *)blobs.data(), *c = (const uint8_t *)comms.data();
        uint32_t st[8], fin[8];
        eth_transcript_blobs_lane(b, n, count, st);
        printf("state "); print_words(st, 8); printf("\n");
        memcpy(fin, st, sizeof fin);
        const uint64_t blocks = eth_transcript_blob_blocks(n, count);
        sha256_lane_resume(eth_transcript_src{b, b, n, count}, 64 * blocks, blocks, fin);
        printf("prefix "); print_words(fin, 8); printf("\n");
        fr r, z;
        eth_transcript_finish_lane(b, c, n, count, st, r, z);
        printf("halves "); print_fr(r); printf(" "); print_fr(z); printf("\n");
        eth_transcript_lane(b, c, n, count, r, z);
        printf("whole "); print_fr(r); printf(" "); print_fr(z); printf("\n");
        return 0;
    }
    fprintf(stderr, "usage: %s resume FILE | transcript N COUNT FILE\n", argv[0]);
    return 2;
}
