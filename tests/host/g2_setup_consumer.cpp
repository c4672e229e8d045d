// g2_setup_consumer.cpp -- GenerateTestingSetup through the C++ mirror of the Go API (include/kzg_hip.hpp), both halves on the device: the G2 half
// compressed with ToCompressedG2 must be the 65 setup_G2 entries of tests/golden/trusted_setup_g2.json ([1337^i] G2), which arrive as lines of hex
// in the file named by argv[1]; the pair then serves the reference's TestKZGSettings_CheckProofSingle scenario (kzg_single_proofs_test.go:36-64).
// TEST INFRASTRUCTURE, built and run by tests/test_gpu_g2_setup.py.  Exit status 0: all equal; 1: a difference; 77: no device.
#include <cstdio>
#include <fstream>
#include <string>
#include "kzg_hip.hpp"

using namespace kzg;

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::vector<std::string> want;
    std::ifstream in(argv[1]);
    for (std::string line; std::getline(in, line);) if (!line.empty()) want.push_back(line);
    if (want.size() != 65) { printf("FAIL fixture: %zu lines\n", want.size()); return 2; }
    if (kzg_hip_device_count() < 1) { printf("no device\n"); return 77; }
    int failures = 0;
    FFTSettings fs(4);
    auto setup = fs.GenerateTestingSetup("1337", 65);
    const std::vector<G1Point> &s1 = setup.first;
    const std::vector<G2Point> &s2 = setup.second;
    if (s1.size() != 65 || s2.size() != 65) { printf("FAIL sizes\n"); return 1; }
    const std::vector<uint8_t> enc = fs.ToCompressedG2(s2);
    static const char d[] = "0123456789abcdef";
    for (size_t i = 0; i < 65; i++) {
        std::string h;
        for (size_t b = 0; b < 96; b++) { h += d[enc[96 * i + b] >> 4]; h += d[enc[96 * i + b] & 15]; }
        if (h != want[i]) { failures++; printf("FAIL setup_G2[%zu]: %s\n", i, h.c_str()); }
    }
    // the G1 half alone gives the same points as the pair's first half
    const std::vector<G1Point> g1 = fs.GenerateTestingSetupG1("1337", 65);
    if (fs.ToCompressedG1(g1) != fs.ToCompressedG1(s1)) { failures++; printf("FAIL G1 half differs\n"); }
    // commit, prove, check: true for y = p(x), false for y + 1
    std::vector<G1Point> s1_17(s1.begin(), s1.begin() + 17);
    std::vector<G2Point> s2_17(s2.begin(), s2.begin() + 17);
    KZGSettings ks(&fs, s1_17);
    ks.SetSecretG2(s2_17);
    std::vector<Fr> poly;
    for (uint64_t v : {1, 2, 3, 4, 7, 7, 7, 7, 13, 13, 13, 13, 13, 13, 13, 13}) poly.push_back(fs.AsFr(v));
    const G1Point c = ks.CommitToPoly(poly), proof = ks.ComputeProofSingle(poly, 3);
    uint64_t y = 0, xp = 1;                                        // p(3) over the integers
    for (uint64_t v : {1, 2, 3, 4, 7, 7, 7, 7, 13, 13, 13, 13, 13, 13, 13, 13}) { y += v * xp; xp *= 3; }
    const std::vector<bool> ok = ks.CheckProofSingleBatch({c, c}, {proof, proof}, {fs.AsFr(3), fs.AsFr(3)}, {fs.AsFr(y), fs.AsFr(y + 1)});
    if (ok.size() != 2 || !ok[0] || ok[1]) { failures++; printf("FAIL CheckProofSingle: %d %d\n", (int)ok[0], (int)ok[1]); }
    printf("%s: %d failure(s)\n", failures ? "FAILED" : "PASSED", failures);
    return failures ? 1 : 0;
}
