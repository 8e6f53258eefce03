"""The Gaussian random stream of ``GP.draw_functions``, restated in vectorised NumPy.

The device (``gpc_draw``, ``gpc_debug_normals``) and the host prior path draw the same numbers:

* Philox4x64-10 with key ``(seed, stream)``; stream 0 feeds the function draws z, stream 1 the noise z'.
* For sample ``s`` (global index), draw ``r`` and row ``j``, with ``q = j // 4``: the row's 64-bit word is lane
  ``j % 4`` of Philox at counter ``(q + 1, r, s, 0)`` -- the first block ``numpy.random.Philox(key=[seed, stream],
  counter=[q, r, s, 0]).random_raw(4)`` returns (NumPy increments the counter before it generates).
* Box-Muller on row pairs ``(2t, 2t + 1)``:
  ``u1 = ((w[2t] >> 11) + 1) 2^-53``, ``u2 = (w[2t+1] >> 11) 2^-53``,
  ``z[2t] = sqrt(-2 ln u1) cos(2 pi u2)``, ``z[2t+1] = sqrt(-2 ln u1) sin(2 pi u2)``.

So a value depends on ``(seed, stream, s, r, j)`` only -- not on M, the number of draws, the samples drawn
together, the chunking or the sharding.
"""

import numpy as np

_M0 = np.uint64(0xD2E7470EE14C6C93)
_M1 = np.uint64(0xCA5A826395121157)
_W0 = np.uint64(0x9E3779B97F4A7C15)
_W1 = np.uint64(0xBB67AE8584CAA73B)
_LO32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhilo(a, b):
    """(hi, lo) of the 128-bit product of uint64 arrays, through 32-bit halves."""
    a_lo, a_hi = a & _LO32, a >> _S32
    b_lo, b_hi = b & _LO32, b >> _S32
    ll = a_lo * b_lo
    lh = a_lo * b_hi
    hl = a_hi * b_lo
    hh = a_hi * b_hi
    mid = (ll >> _S32) + (lh & _LO32) + (hl & _LO32)
    hi = hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)
    return hi, a * b


def philox4x64_10(ctr, key):
    """Philox4x64-10 of counters ``ctr`` (4 uint64 arrays, broadcastable) under ``key`` (2 uint64 scalars or arrays):
    the four output words."""
    with np.errstate(over="ignore"):
        c0, c1, c2, c3 = (np.asarray(x, dtype=np.uint64) for x in ctr)
        k0, k1 = (np.asarray(x, dtype=np.uint64) for x in key)
        for rnd in range(10):
            if rnd:
                k0 = k0 + _W0
                k1 = k1 + _W1
            hi0, lo0 = _mulhilo(_M0, c0)
            hi1, lo1 = _mulhilo(_M1, c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def _check_seed(seed):
    seed = int(seed)
    if not 0 <= seed < 2**64:
        raise ValueError(f"seed must lie in [0, 2**64), got {seed}")
    return seed


def words(seed, stream, s, r, j):
    """The 64-bit words of rows ``j`` (int array) for sample ``s`` and draw ``r`` (ints or arrays broadcastable
    with ``j``): lane j % 4 of Philox at counter (j // 4 + 1, r, s, 0) under key (seed, stream)."""
    seed = _check_seed(seed)
    j = np.asarray(j, dtype=np.int64)
    q = (j // 4).astype(np.uint64) + np.uint64(1)
    s = np.asarray(s, dtype=np.uint64)
    r = np.asarray(r, dtype=np.uint64)
    out = philox4x64_10((q, r, s, np.uint64(0)), (np.uint64(seed), np.uint64(stream)))
    shape = np.broadcast(q, r, s).shape
    lanes = np.stack([np.broadcast_to(w, shape) for w in out])
    lane = np.broadcast_to(j % 4, shape)
    return np.take_along_axis(lanes, lane[None], 0)[0]


def box_muller(w_even, w_odd):
    """The two normals of a row pair from its two words (uint64 arrays)."""
    u1 = ((np.asarray(w_even, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0**-53
    u2 = (np.asarray(w_odd, dtype=np.uint64) >> np.uint64(11)).astype(np.float64) * 2.0**-53
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return rad * np.cos(ang), rad * np.sin(ang)


def normals(seed, stream, s, r, j):
    """Standard normals z[j] of sample ``s`` (int or array) and draw ``r`` (int or array) at rows ``j`` (int array),
    broadcast together.  Row j pairs with j ^ 1."""
    j = np.asarray(j, dtype=np.int64)
    even = j & ~np.int64(1)
    z0, z1 = box_muller(words(seed, stream, s, r, even), words(seed, stream, s, r, even + 1))
    return np.where(j & 1, z1, z0)


def normals_block(seed, stream, M, R, s_idx):
    """z of shape (M, R, len(s_idx)): rows 0..M-1, draws 0..R-1, the global sample indices ``s_idx``."""
    s_idx = np.asarray(s_idx, dtype=np.int64).reshape(1, 1, -1)
    j = np.arange(M).reshape(-1, 1, 1)
    r = np.arange(R).reshape(1, -1, 1)
    return normals(seed, stream, s_idx, r, j)
