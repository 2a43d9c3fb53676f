"""What the pack tests share: the scalar rule of the three bit planes in numpy -- the reference's code table
(dna_text.c:41-46: A C G T in either case, everything else code 4), a byte at a time, nothing of qe_pack.h -- and the inputs
of tests/test_gpu_pack_planes.py.  Test infrastructure only."""
import numpy as np

FLAG_HAS_N, FLAG_NONCANON = 1, 2
# lengths across every boundary of the scheme: 16-byte lane spans, 64-base rows, 1 KB wave spans, the first spans that are
# loaded with no guard (1024, 2048, 4096 = one full trip of four) and the ones around them
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1007, 1008, 1009, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4097)

# the planes' base code: ASCII bits 1 and 2 of the letter (A 0, C 1, T 2, G 3); 4 = not a base
CODE = np.full(256, 4, dtype=np.uint8)
for _letter, _code in ((b"A", 0), (b"C", 1), (b"T", 2), (b"G", 3)):
    CODE[_letter[0]] = CODE[_letter.lower()[0]] = _code
UPPER = np.zeros(256, dtype=bool)
for _c in b"ACGT":
    UPPER[_c] = True


def rows_of(length):
    return (length + 63) // 64 + 2


def ref_pack(seq, reverse=False):
    """-> (uint64 words [rows][3] flattened, flags) of one sequence"""
    b = np.frombuffer(seq, dtype=np.uint8)
    if reverse:
        b = b[::-1]
    code = CODE[b]
    rows = rows_of(len(b))
    bits = np.zeros((rows * 64, 3), dtype=np.uint8)
    base = code < 4
    bits[:len(b), 0] = (code & 1) * base
    bits[:len(b), 1] = (code >> 1) * base
    bits[:len(b), 2] = ~base
    words = np.packbits(bits.reshape(rows, 64, 3).transpose(0, 2, 1), axis=-1, bitorder="little").reshape(rows * 3, 8)
    words = np.ascontiguousarray(words).view("<u8").reshape(-1)
    flags = 0
    if (~base).any():
        flags |= FLAG_HAS_N
    if (base & ~UPPER[b]).any() or (~base & (b != ord("N"))).any():
        flags |= FLAG_NONCANON
    return words.astype(np.uint64), flags


def ref_pack_set(seqs, reverse=False):
    """-> (words of the set back to back, word offsets, flags per sequence): the library's layout of a set"""
    words, off, flags, top = [], [], [], 0
    for s in seqs:
        w, f = ref_pack(s, reverse)
        off.append(top)
        top += len(w)
        words.append(w)
        flags.append(f)
    return (np.concatenate(words) if words else np.zeros(0, dtype=np.uint64)), np.array(off, dtype=np.int64), np.array(flags, dtype=np.uint32)


def sequences(seed=7):
    """every length of LENGTHS in six alphabets, and all 256 byte values at every position of a 16-byte lane"""
    rng = np.random.default_rng(seed)
    alphabets = [b"ACGT", b"ACGTacgt", b"ACGTACGTACGTNn", b"ACGTRYSWKMBDHVNUryswkmbdhvnu", b"ACGTacgt" + bytes([0x00, 0x7F, 0x80, 0xFF]),
                 bytes(range(256))]
    out = []
    for alpha in alphabets:
        a = np.frombuffer(alpha, dtype=np.uint8)
        for n in LENGTHS:
            out.append(a[rng.integers(0, len(a), size=n)].tobytes())
    for pos in range(16):
        for v in range(256):
            s = bytearray(b"ACGTTGCAACGTTGCA")
            s[pos] = v
            out.append(bytes(s))
    return out
