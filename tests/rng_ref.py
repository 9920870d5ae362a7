"""The counter-based dropout RNG of csrc/common.h restated in plain numpy integer arithmetic.

Written from the documented algorithm, never calling the library: the device kernels are compared against THIS, so a
defect in the hash, the 16-bit field selection, the threshold or the 64-bit index folding cannot sit in a kernel and in
its reference alike.

  key    = mix32(mix32(lo32(seed) ^ 0x9e3779b9) ^ hi32(seed) ^ site * 0x632be5ab)          (all mod 2^32)
  group  g = element >> 2 (64 bit), lo = lo32(g), hi = hi32(g)
  w0     = mix32(key ^ lo ^ rot16(hi) ^ hi)
  w1     = t ^ (t >> 13),  t = (w0 ^ (w0 >> 15)) * 0x2c1b3c6d
  field  of sub-position s = element & 3:  s = 0: w0 & 0xFFFF, 1: w0 >> 16, 2: w1 & 0xFFFF, 3: w1 >> 16
  keep   = field >= uint32(float32(p) * 65536.0f)
  mix32  = the murmur3 finaliser: h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16
"""
import numpy as np

U32 = np.uint32
U64 = np.uint64
M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF

SITE_CONV = 16                  # conv layer l, node type ti: SITE_CONV + 8 * l + ti
SITE_H1, SITE_H2 = 64, 65       # the pair heads' two dropout layers
SITE_SUP = 0x53555031           # the supervision subset


def _mix32(h):
    """murmur3 finaliser on a uint32 array (numpy integer arrays wrap mod 2^32)."""
    h = h ^ (h >> U32(16))
    h = h * U32(0x85EBCA6B)
    h = h ^ (h >> U32(13))
    h = h * U32(0xC2B2AE35)
    return h ^ (h >> U32(16))


def _mix32_int(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def key(seed, site):
    """(seed mod 2^64, site mod 2^32) -> the 32-bit key, a Python int."""
    seed, site = int(seed) & M64, int(site) & M32
    h = _mix32_int((seed & M32) ^ 0x9E3779B9)
    return _mix32_int(h ^ (seed >> 32) ^ ((site * 0x632BE5AB) & M32))


def group_words(k, grp):
    """key, uint64 array of group indices -> (w0, w1) uint32 arrays."""
    grp = np.asarray(grp, dtype=U64)
    lo = (grp & U64(M32)).astype(U32)
    hi = (grp >> U64(32)).astype(U32)
    rot = (hi << U32(16)) | (hi >> U32(16))
    w0 = _mix32(U32(int(k) & M32) ^ lo ^ rot ^ hi)
    t = (w0 ^ (w0 >> U32(15))) * U32(0x2C1B3C6D)
    return w0, t ^ (t >> U32(13))


def fields_at(k, elems):
    """key, uint64 array of element indices (any shape, any order) -> their 16-bit fields (uint32 array)."""
    elems = np.asarray(elems, dtype=U64)
    w0, w1 = group_words(k, elems >> U64(2))
    sub = (elems & U64(3)).astype(U32)
    word = np.where((sub & U32(2)) != 0, w1, w0)
    return (word >> ((sub & U32(1)) * U32(16))) & U32(0xFFFF)


def fields(seed, site, first, n):
    """The 16-bit fields of elements first .. first + n - 1 (first: a Python int below 2^64)."""
    first, n = int(first), int(n)
    g0 = first >> 2
    ng = ((first + n + 3) >> 2) - g0                       # one hash per group of four, as the kernels share it
    w0, w1 = group_words(key(seed, site), U64(g0) + np.arange(ng, dtype=U64))
    four = np.stack([w0 & U32(0xFFFF), w0 >> U32(16), w1 & U32(0xFFFF), w1 >> U32(16)], axis=1).ravel()
    return four[first & 3:(first & 3) + n]


def threshold(p):
    """uint32(float32(p) * 65536.0f): the product is exact in float32 (a power of two), the conversion truncates."""
    return int(np.float32(p) * np.float32(65536.0))


def inv_keep(p):
    """The factor a kept element is scaled by: 1.0f / (1.0f - float32(p)) in float32 arithmetic."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_at(seed, site, elems, p):
    return fields_at(key(seed, site), elems) >= U32(threshold(p))


def keep(seed, site, first, n, p):
    """Boolean keep decisions of elements first .. first + n - 1: kept with probability 1 - threshold(p) / 65536."""
    return fields(seed, site, first, n) >= U32(threshold(p))


def mask2d(seed, site, n_rows, width, p, row_offset=0):
    """The keep-mask ([n_rows, width] bool) of a row-major tensor whose row 0 is global row `row_offset`: element
    (r, c) is element (row_offset + r) * width + c of the stream."""
    return keep(seed, site, int(row_offset) * int(width), int(n_rows) * int(width), p).reshape(int(n_rows), int(width))


def splitmix(state):
    """One step of the seed stream: state = (published seed, position) as Python ints mod 2^64 -> the next state.
    SplitMix64 on the position; the published seed is the output >> 2 (it stays a non-negative int64)."""
    pos = (int(state[1]) + 0x9E3779B97F4A7C15) & M64
    z = pos
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return ((z ^ (z >> 31)) >> 2, pos)
