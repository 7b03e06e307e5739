"""References for sample-rate conversion (csrc/resample.hpp), in long double, the cases the GPU tests
share, and a numpy model of the polyphase kernel's schedule.  A plain helper, not a test.

    upfirdn_ref        full[m] = sum_n h[m down - n up] x[n] in its polyphase form, with sum |h x| per output (the gate's scale)
    firwin_ref         the windowed-sinc low-pass, unit sum
    resample_poly_ref  scipy's recipe on top of upfirdn_ref
    decimate_ref       the FIR, zero-phase form
    resample_ref       the Fourier method
    geom / upfirdn_model   upfirdn_geom of resample.hpp and the kernel's tiles, tap chunks, phase-major table and order
"""
import math

import numpy as np

LD = np.longdouble
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
NDT = {"f64": np.float64, "f32": np.float32}

# the constants of csrc/resample.hpp
TAP_LDS, SIG_LDS, MAX_TILE, MAX_ROWS = 4096, 4096, 1024, 256

# (L, K, up, down)
UPFIRDN_CASES = [
    (1, 1, 1, 1),
    (5, 3, 5, 1),           # phases without taps
    (17, 7, 3, 2),
    (40, 33, 2, 3),
    (9, 4, 1, 7),
    (3, 50, 4, 5),          # K >> L
    (300, 3201, 160, 147),  # the 44.1 -> 48 kHz filter of resample_poly
    (300, 3201, 147, 160),  # and back
    (40, 4200, 7, 5),       # Kp = 600 > the chunk of 585: two tap chunks of phase rows
    (20, 6000, 300, 7),     # up > 256: a row per output, Kp = 20 > the chunk of 16
    (4096, 5000, 1, 1),     # K exceeds the whole LDS table: three chunks of one row
]
# (L, num)
FOURIER_CASES = [(1, 1), (1, 5), (5, 1), (8, 8), (8, 5), (8, 6), (8, 12), (8, 13), (9, 4), (9, 6), (9, 14), (2, 1), (6, 4),
                 (1000, 441), (441, 1000), (8209, 4096)]  # 8209 is prime: Bluestein in, a power of two out


def full_len(L, K, up, down):
    return ((L - 1) * up + K - 1) // down + 1


def kp_of(K, up):
    return -(-K // up)


def phase_table(h, up, stride=None):
    """up rows of Kp taps (`stride` apart: the device table's Kp | 1), row p = h[p], h[p + up], ..., zeros behind"""
    h = np.asarray(h)
    K = h.size
    kp = kp_of(K, up)
    tab = np.zeros((up, kp if stride is None else stride), h.dtype)
    i = np.arange(K)
    tab[i % up, i // up] = h
    return tab


def upfirdn_ref(h, x, up, down, first=0, out_len=None):
    """(out, scale): out[i] = full[first + i] in long double from the values as given, and scale[i] = sum |h x| of it.
    Samples beyond full_len are 0."""
    h, x = np.asarray(h).astype(LD), np.asarray(x).astype(LD)
    L, K = x.size, h.size
    n_full = full_len(L, K, up, down)
    if out_len is None:
        out_len = n_full - first
    kp = kp_of(K, up)
    tab = phase_table(h, up)
    m = first + np.arange(out_len, dtype=np.int64)
    p, q = (m * down) % up, (m * down) // up
    out, scale = np.zeros(out_len, LD), np.zeros(out_len, LD)
    for j in range(kp):
        n = q - j
        ok = (n >= 0) & (n < L)
        term = np.where(ok, tab[p, j] * x[np.clip(n, 0, L - 1)], LD(0))
        out += term
        scale += np.abs(term)
    return out, scale


def products(K, up):
    """the products of an output's sum in the kernel: Kp"""
    return kp_of(K, up)


def window_ref(name, n):
    k = np.arange(n, dtype=LD)
    if name == "hamming":
        return LD(0.54) - LD(0.46) * np.cos(2 * LD(np.pi) * k / (n - 1)) if n > 1 else np.ones(1, LD)
    if isinstance(name, tuple) and name[0] == "kaiser":
        return np.kaiser(n, name[1]).astype(LD)  # (np.i0 is double: the window is double-accurate, as scipy's is)
    raise ValueError(name)


def firwin_ref(numtaps, cutoff, window=("kaiser", 5.0)):
    m = np.arange(numtaps, dtype=LD) - LD(numtaps - 1) / 2
    arg = LD(np.pi) * LD(cutoff) * m
    sinc = np.where(m == 0, LD(1), np.sin(arg) / np.where(m == 0, LD(1), arg))
    h = LD(cutoff) * sinc * window_ref(window, numtaps)
    return h / h.sum()


def resample_poly_plan(L, up, down, taps=None, window=("kaiser", 5.0)):
    """(h with its leading zeros, up, down, first, n_out) of scipy's recipe; taps: an array instead of a window"""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    n_out = -(-L * up // down)
    if taps is None:
        half = 10 * max(up, down)
        taps = firwin_ref(2 * half + 1, 1.0 / max(up, down), window)
    else:
        taps = np.asarray(taps).astype(LD)
        half = (taps.size - 1) // 2
    pre = down - half % down
    h = np.concatenate((np.zeros(pre, LD), taps * up))
    return h, up, down, (half + pre) // down, n_out


def resample_poly_ref(x, up, down, taps=None, window=("kaiser", 5.0)):
    h, up, down, first, n_out = resample_poly_plan(len(x), up, down, taps, window)
    if up == down == 1:
        return np.asarray(x).astype(LD)
    return upfirdn_ref(h, x, up, down, first, n_out)[0]


def decimate_ref(x, q, n=None):
    n = 20 * q if n is None else n
    return resample_poly_ref(x, 1, q, taps=firwin_ref(n + 1, 1.0 / q, "hamming"))


def resample_ref(x, num):
    x = np.asarray(x).astype(LD)
    L = x.size
    X = np.fft.rfft(x)
    N = min(L, num)
    Y = np.zeros(num // 2 + 1, X.dtype)
    Y[:N // 2 + 1] = X[:N // 2 + 1]
    if N % 2 == 0:
        if num < L:
            Y[N // 2] *= 2
        elif num > L:
            Y[N // 2] *= LD(0.5)
    return np.fft.irfft(Y, num) * (LD(num) / LD(L))


# ---- the kernel's schedule ----
def geom(K, up, down):
    """upfirdn_geom: (rows, jc, stride, tile, by_phase)"""
    kp = kp_of(K, up)
    by_phase = up <= MAX_ROWS
    rows = up if by_phase else MAX_ROWS
    jc = min(TAP_LDS // rows, SIG_LDS // 2, kp)
    tile = min(1 + (SIG_LDS - jc) * up // down, MAX_TILE if by_phase else MAX_ROWS)
    return rows, jc, jc | 1, tile, by_phase


def _fma(a, b, c, dtype):
    """fma in dtype: exact for f32 through double (24 + 24 bits); for f64 the product is exact on the integer-valued data the
    bit tests use, and rounds once more on random data (inside the gate all the same)"""
    if dtype == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def upfirdn_model(h, x, up, down, first=0, out_len=None, dtype=np.float64):
    """the kernel, tile by tile and chunk by chunk, with its LDS arrays: the bits of the device (fma as _fma says)"""
    h, x = np.asarray(h, dtype), np.asarray(x, dtype)
    L, K = x.size, h.size
    if out_len is None:
        out_len = full_len(L, K, up, down) - first
    kp = kp_of(K, up)
    ts = kp | 1
    table = phase_table(h, up, ts).reshape(-1)
    rows, jc, stride, tile, by_phase = geom(K, up, down)
    out = np.full(out_len, np.nan, dtype)
    for i0 in range(0, out_len, tile):
        n = min(tile, out_len - i0)
        m = first + i0 + np.arange(n, dtype=np.int64)
        q, p = (m * down) // up, (m * down) % up
        q0 = int(q[0])
        span = int(q[-1]) - q0 + jc
        assert span <= SIG_LDS and n <= (MAX_TILE if by_phase else MAX_ROWS)
        row = (p if by_phase else np.arange(n)) * stride
        assert row.max() + jc <= TAP_LDS + 512
        acc = np.zeros(n, dtype)
        for j0 in range(0, kp, jc):
            jn = min(jc, kp - j0)
            taps = np.full(TAP_LDS + 512, np.nan, dtype)  # what is not staged must not be read
            sig = np.full(SIG_LDS, np.nan, dtype)
            if by_phase and jc == kp:   # one chunk: the table's rows are `stride` apart, a straight copy
                assert stride == ts
                taps[:rows * stride] = table
            elif by_phase:
                for r in range(rows):
                    taps[r * stride:r * stride + jn] = table[r * ts + j0:r * ts + j0 + jn]
            else:
                for i in range(n):
                    taps[row[i]:row[i] + jn] = table[p[i] * ts + j0:p[i] * ts + j0 + jn]
            lo = q0 - (j0 + jc - 1)
            s = lo + np.arange(span)
            ok = (s >= 0) & (s < L)
            sig[:span] = np.where(ok, x[np.clip(s, 0, L - 1)], dtype(0))
            for jj in range(jn):
                acc = _fma(taps[row + jj], sig[(q - q0) + (jc - 1) - jj], acc, dtype)
        out[i0:i0 + n] = acc
    return out


def signal(L, dt, seed=0, batch=None):
    rng = np.random.default_rng([seed, L, 27])
    return rng.uniform(-1, 1, L if batch is None else (batch, L)).astype(NDT[dt])


def taps(K, dt, seed=0):
    return np.random.default_rng([seed, K, 28]).uniform(-1, 1, K).astype(NDT[dt])


def poly_gate(dt, K, up, scale):
    """|got - ref| <= (n + 2) u sum |h x| for a sum of n = Kp products in any order"""
    return (products(K, up) + 2) * U[dt] * np.asarray(scale, np.float64)


def inner_m(n):
    """the length whose log2 the Fourier gates use: as tests/test_gpu_any_real.py"""
    if n & (n - 1) == 0:
        return n
    m = n if n & 1 else n // 2
    return m if m & (m - 1) == 0 else 1 << (2 * m - 2).bit_length()


def fourier_log2(L, num):
    return max(inner_m(L), inner_m(num)).bit_length() - 1
