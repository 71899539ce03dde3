"""numpy model of the two-bit transport of FASTA bases (mumemto_amd/csrc/base_pack.hpp, k::unpack_bases): what the host
packer makes of a chunk and what the device must write back.  tests/test_base_pack_host.py holds it to the byte loop of
tests/base_pack_check.cpp; tests/test_gpu_packed_input.py holds the kernel to it."""
import numpy as np

_CODE = np.full(256, 4, np.uint8)
for _i, _pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    for _b in _pair:
        _CODE[_b] = _i
_ASCII = np.frombuffer(b"ACGT", np.uint8)
_SHIFT = (2 * np.arange(32)).astype(np.uint64)


def pack(bases):
    """bases: uint8 array -> (words uint64[(n + 31) // 32], runs uint32[k, 3] of (start, length, byte))"""
    bases = np.ascontiguousarray(bases, np.uint8)
    n = len(bases)
    code = _CODE[bases]
    exc = code == 4
    padded = np.zeros((n + 31) // 32 * 32, np.uint64)
    padded[:n] = np.where(exc, 0, code)
    words = np.bitwise_or.reduce(padded.reshape(-1, 32) << _SHIFT, axis=1) if n else np.zeros(0, np.uint64)
    # a run starts at an exception byte whose predecessor is not the same exception byte
    first = exc.copy()
    first[1:] &= ~(exc[:-1] & (bases[:-1] == bases[1:]))
    last = exc.copy()
    last[:-1] &= ~(exc[1:] & (bases[:-1] == bases[1:]))
    start, end = np.flatnonzero(first), np.flatnonzero(last) + 1
    runs = np.stack([start, end - start, bases[start]], axis=1).astype(np.uint32) if len(start) else np.zeros((0, 3), np.uint32)
    return words.astype(np.uint64), runs


def unpack(words, n, runs):
    """the n bytes the device writes: A C G T from the codes, then the runs over them"""
    codes = ((np.asarray(words, np.uint64)[:, None] >> _SHIFT) & np.uint64(3)).reshape(-1)[:n].astype(np.intp)
    out = _ASCII[codes].copy()
    for s, l, b in np.asarray(runs, np.uint32).reshape(-1, 3):
        out[int(s):int(s) + int(l)] = b
    return out


def contents(n, seed=1):
    """the content classes of the issue at length n: name -> uint8 array"""
    rng = np.random.default_rng(seed + n)
    pick = lambda alphabet: np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].copy()  # noqa: E731
    wild = b"ACGTNnRYKMSWBDHVryu*-" + bytes(range(0x80, 0x100, 9))
    out = {"one base": np.full(n, ord("G"), np.uint8), "ACGTacgt": pick(b"ACGTacgt"), "wild": pick(wild)}
    v = pick(b"ACGT")
    if n:
        v[0] = ord("N"); v[-1] = ord("x")
    out["exception at both ends"] = v
    v = pick(b"ACGTacgt")
    v[20:45] = ord("N"); v[60:100] = ord("n"); v[4090:4100] = ord("N")
    out["runs across words"] = v
    v = pick(b"ACGT")
    v[10:15] = ord("N"); v[15:20] = ord("n"); v[30:32] = ord("R"); v[32:40] = ord("Y"); v[40:41] = ord("N")
    out["adjacent runs"] = v
    out["one run"] = np.full(n, ord("N"), np.uint8)
    return out
