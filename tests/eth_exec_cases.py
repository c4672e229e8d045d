"""Python restatement of the execution-layer side of eth/eth.go (KZGToVersionedHash, TxPeekBlobVersionedHashes,
VerifyKZGCommitmentsAgainstTransactions) with the result codes of include/kzg_hip.h, and builders of serialized transactions and blocks for
the tests.  A plain helper module, imported by name from tests/test_eth_exec_host.py (host) and tests/test_gpu_eth_exec.py (device).  Nothing
here calls the library: expectations come from hashlib and Python integers."""
import hashlib

VALID, HASH_MISMATCH, COUNT_MISMATCH, TX_TOO_SHORT, TX_OFFSET, TX_TRAILING = 1, 4, 5, 6, 7, 8
BLOB_TX_TYPE = 5
HASHES_OFFSET_FIELD = 258          # position of the offset to the versioned hashes in a serialized blob transaction (eth/eth.go:68)
MESSAGE_START = 70                 # the offset counts from the start of the "message"
MIN_OFFSET = HASHES_OFFSET_FIELD + 4 - MESSAGE_START   # 192: the hashes follow the fixed part at once


def versioned_hash(commitment48):
    """KZGToVersionedHash (eth/eth.go:137-141)"""
    return bytes([0x01]) + hashlib.sha256(bytes(commitment48)).digest()[1:]


def tx_peek(tx):
    """(code, first, count) as tx_peek_blob_versioned_hashes (go-kzg_amd/csrc/eth_tx.hpp) returns them: code 0 and the hashes at
    tx[first : first + 32 count], or 6 / 7 / 8; restates eth/eth.go:234-256 behind the caller's type check (eth/eth.go:264)"""
    if len(tx) == 0:
        return TX_TOO_SHORT, 0, 0                          # the reference panics on tx[0]
    if tx[0] != BLOB_TX_TYPE:
        return 0, 0, 0                                     # skipped
    if len(tx) < HASHES_OFFSET_FIELD + 4:
        return TX_TOO_SHORT, 0, 0
    offset = int.from_bytes(tx[HASHES_OFFSET_FIELD:HASHES_OFFSET_FIELD + 4], "little") + MESSAGE_START
    if offset > len(tx):
        return TX_OFFSET, 0, 0
    if (len(tx) - offset) % 32:
        return TX_TRAILING, 0, 0
    return 0, offset, (len(tx) - offset) // 32


def verify_block(txs, commitments):
    """VerifyKZGCommitmentsAgainstTransactions (eth/eth.go:261-282) as a code: the first malformed blob transaction, then the counts, then
    the hashes"""
    hashes = []
    for tx in txs:
        code, first, count = tx_peek(tx)
        if code:
            return code
        hashes += [tx[first + 32 * i:first + 32 * i + 32] for i in range(count)]
    if len(hashes) != len(commitments):
        return COUNT_MISMATCH
    for h, c in zip(hashes, commitments):
        if versioned_hash(c) != h:
            return HASH_MISMATCH
    return VALID


def blob_tx(hashes, rng, dynamic=0, offset=None, tx_type=BLOB_TX_TYPE, trailing=b""):
    """a serialized transaction: type byte, 257 arbitrary bytes, the offset field, `dynamic` arbitrary bytes of other dynamic data, the hashes,
    `trailing` extra bytes.  offset: the field's value (default: where the hashes start, 192 + dynamic)"""
    field = MIN_OFFSET + dynamic if offset is None else offset
    return (bytes([tx_type]) + rng.randbytes(HASHES_OFFSET_FIELD - 1) + field.to_bytes(4, "little") + rng.randbytes(dynamic) + b"".join(hashes) + trailing)


def other_tx(rng, length, tx_type=2):
    """a transaction of another type (any length >= 1): skipped whatever it holds"""
    return bytes([tx_type]) + rng.randbytes(length - 1)


def commitments(rng, k):
    """k arbitrary 48-byte strings: the check hashes before anything decodes"""
    return [rng.randbytes(48) for _ in range(k)]


def spread(hashes, rng, parts):
    """the hashes cut into `parts` blob transactions with different amounts of other dynamic data, transactions of other types between them"""
    cuts = sorted(rng.randrange(len(hashes) + 1) for _ in range(parts - 1))
    txs = [other_tx(rng, 1)]
    for k, (a, b) in enumerate(zip([0] + cuts, cuts + [len(hashes)])):
        txs.append(blob_tx(hashes[a:b], rng, dynamic=(0, 7, 64, 333)[k % 4]))
        txs.append(other_tx(rng, rng.randrange(1, 400), tx_type=(0, 2, 1)[k % 3]))
    return txs


def named_blocks(rng):
    """[(name, transactions, commitments)]: every shape the check distinguishes"""
    out = []
    good = lambda k: (lambda c: (c, [versioned_hash(x) for x in c]))(commitments(rng, k))
    out.append(("empty", [], []))
    out.append(("no_blob_txs", [other_tx(rng, 300), other_tx(rng, 1), other_tx(rng, 262, tx_type=0)], []))
    c, h = good(5)
    out.append(("spread", spread(h, rng, 3), c))
    c, h = good(2)
    out.append(("zero_hash_tx", [blob_tx([], rng, dynamic=9), blob_tx(h, rng), blob_tx([], rng)], c))
    c, h = good(1)
    out.append(("minimal_offset", [blob_tx(h, rng, dynamic=0)], c))
    c, h = good(3)
    out.append(("dynamic_data", [blob_tx(h, rng, dynamic=1000)], c))
    c, h = good(3)
    out.append(("count+1", [blob_tx(h, rng)], c + commitments(rng, 1)))
    out.append(("count-1", [blob_tx(h, rng)], c[:2]))
    out.append(("hashes_without_commitments", [blob_tx(h, rng)], []))
    c, h = good(4)
    for name, k in (("first", 0), ("middle", 2), ("last", 3)):
        bad = list(h)
        bad[k] = bad[k][:13] + bytes([bad[k][13] ^ 0x40]) + bad[k][14:]
        out.append(("wrong_hash_" + name, spread(bad, rng, 2), c))
    out.append(("raw_digest", [blob_tx([hashlib.sha256(x).digest() for x in c], rng)], c))
    short = blob_tx(h, rng)[:261]
    beyond = blob_tx(h, rng, offset=MIN_OFFSET + 32 * 4 + 1)
    ragged = blob_tx(h, rng, trailing=b"\x00" * 5)
    out.append(("too_short", [blob_tx(h, rng), short], c + c))
    out.append(("offset_out_of_bounds", [beyond], c))
    out.append(("trailing", [ragged], c))
    out.append(("empty_tx", [other_tx(rng, 20), b"", blob_tx(h, rng)], c))
    out.append(("two_malformations_7_then_6", [other_tx(rng, 5), beyond, short], c))
    out.append(("two_malformations_8_then_7", [ragged, beyond], c))
    wrong = [h[1]] + h[1:]
    out.append(("malformed+count+hash", [blob_tx(wrong, rng), short], c[:1]))
    out.append(("count+hash", [blob_tx(wrong, rng)], c[:3]))
    return out


def ragged_blocks(rng, n):
    """n blocks with 0 .. 6 commitments each (block boundaries fall inside wavefronts); every seventh has its last hash spoiled, every
    eleventh a commitment too many, every thirteenth a malformed transaction: a bad block between good ones"""
    out = []
    for j in range(n):
        k = (j * 5 + j // 7) % 7
        c = commitments(rng, k)
        h = [versioned_hash(x) for x in c]
        if j % 7 == 3 and k:
            h[-1] = h[-1][:31] + bytes([h[-1][31] ^ 1])
        txs = spread(h, rng, 1 + j % 3) if k else ([other_tx(rng, 3)] if j % 2 else [])
        if j % 11 == 5:
            c = c + commitments(rng, 1)
        if j % 13 == 6:
            txs = txs + [blob_tx(h, rng, trailing=b"\x01")]
        out.append((txs, c))
    return out
