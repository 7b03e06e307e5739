"""Long-double reference of the discrete wavelet transform (include/phastft_hip.h): PyWavelets' definitions
written out, one function per formula, over the taps and samples as the device gets them (rounded to T by the caller).

    ext_index        the extension map: the index of ext(x, t), or -1 for a zero
    analysis_level   cA[i] = sum_j dec_lo[j] ext(x, 2i + 1 - j)         (periodization: x[(2i + F/2 - j) mod n'])
    synthesis_level  y[r]  = sum_k rec_lo[r + F - 2 - 2k] cA[k] + rec_hi[..] cD[k]   (periodization: taps t = r + F/2 - 1 - 2k mod N)
    wavedec / waverec  the cascade; waverec keeps the first n_{l-1} samples of each level
    abs_*            the absolute cascade: the same sums with |taps| on |values| -- the scale of the rounding-error gates

The sums over the taps are numpy long-double dot products of gathered rows; nothing here shares code with the library."""
import numpy as np

LD = np.longdouble
MODES = ("zero", "constant", "symmetric", "reflect", "periodic", "periodization")


def ext_index(mode: str, n: int, t):
    """index of ext(x, t) for integer (array) t and a signal of n samples; -1 where the extension is zero"""
    t = np.asarray(t, dtype=np.int64)
    if mode == "zero":
        return np.where((t >= 0) & (t < n), t, -1)
    if mode == "constant":
        return np.clip(t, 0, n - 1)
    if mode == "periodic":
        return np.mod(t, n)
    if mode == "symmetric":
        u = np.mod(t, 2 * n)
        return np.where(u < n, u, 2 * n - 1 - u)
    if mode == "reflect":
        if n == 1:
            return np.zeros_like(t)
        u = np.mod(t, 2 * n - 2)
        return np.where(u < n, u, 2 * n - 2 - u)
    if mode == "periodization":
        u = np.mod(t, n + n % 2)
        return np.minimum(u, n - 1)   # x[n] := x[n - 1] for odd n
    raise ValueError(mode)


def level_len(n: int, f: int, mode: str) -> int:
    return (n + n % 2) // 2 if mode == "periodization" else (n + f - 1) // 2


def synth_len(m: int, f: int, mode: str) -> int:
    return 2 * m if mode == "periodization" else 2 * m - f + 2


def level_lens(L: int, f: int, level: int, mode: str):
    """[n_0, .., n_J]"""
    out = [L]
    for _ in range(level):
        out.append(level_len(out[-1], f, mode))
    return out


def max_level(L: int, f: int) -> int:
    j = 0
    while L // (1 << (j + 1)) >= f - 1:
        j += 1
    return j


def _gather(x, idx):
    x = np.asarray(x, dtype=LD)
    return np.where(idx >= 0, x[np.maximum(idx, 0)], LD(0))


def analysis_level(x, dec_lo, dec_hi, mode: str):
    x, dec_lo, dec_hi = (np.asarray(v, dtype=LD) for v in (x, dec_lo, dec_hi))
    n, f = x.size, dec_lo.size
    m = level_len(n, f, mode)
    i = np.arange(m, dtype=np.int64)[:, None]
    j = np.arange(f, dtype=np.int64)[None, :]
    t = 2 * i + (f // 2 if mode == "periodization" else 1) - j
    rows = _gather(x, ext_index(mode, n, t))
    return (rows * dec_lo[None, :]).sum(axis=1), (rows * dec_hi[None, :]).sum(axis=1)


def synthesis_level(cA, cD, rec_lo, rec_hi, mode: str):
    cA, cD, rec_lo, rec_hi = (np.asarray(v, dtype=LD) for v in (cA, cD, rec_lo, rec_hi))
    m, f = cA.size, rec_lo.size
    N = synth_len(m, f, mode)
    if N < 1:
        raise ValueError("too few coefficients for this filter")
    r = np.arange(N, dtype=np.int64)[:, None]
    t = np.arange(f, dtype=np.int64)[None, :]
    num = r + (f // 2 - 1 if mode == "periodization" else f - 2) - t    # 2k
    k = num // 2
    ok = num % 2 == 0
    if mode == "periodization":
        k = np.mod(k, m)     # every integer k' counts: more than one tap per coefficient when F > N
    else:
        ok &= (k >= 0) & (k < m)
    idx = np.where(ok, k, -1)
    return (_gather(cA, idx) * rec_lo[None, :]).sum(axis=1) + (_gather(cD, idx) * rec_hi[None, :]).sum(axis=1)


def wavedec(x, bank, level: int, mode: str):
    """[cA_J, cD_J, .., cD_1] in long double"""
    dec_lo, dec_hi = bank[0], bank[1]
    a, details = np.asarray(x, dtype=LD), []
    for _ in range(level):
        a, d = analysis_level(a, dec_lo, dec_hi, mode)
        details.append(d)
    return [a] + details[::-1]


def waverec(coeffs, bank, mode: str, signal_len: int):
    """the signal of signal_len samples: at every level the first n_{l-1} of the reconstructed samples are kept"""
    rec_lo, rec_hi = bank[2], bank[3]
    f, level = np.asarray(rec_lo).size, len(coeffs) - 1
    lens = level_lens(signal_len, f, level, mode)
    a = np.asarray(coeffs[0], dtype=LD)
    for l in range(level, 0, -1):
        d = np.asarray(coeffs[level - l + 1], dtype=LD)
        assert a.size == d.size == lens[l], (a.size, d.size, lens[l])
        y = synthesis_level(a, d, rec_lo, rec_hi, mode)
        assert y.size in (lens[l - 1], lens[l - 1] + 1), (y.size, lens[l - 1])
        a = y[:lens[l - 1]]
    return a


def pack(coeffs):
    return np.concatenate([np.asarray(c, dtype=LD) for c in coeffs])


def unpack(packed, L: int, f: int, level: int, mode: str):
    lens = level_lens(L, f, level, mode)
    sizes = [lens[level]] + [lens[l] for l in range(level, 0, -1)]
    out, at = [], 0
    for s in sizes:
        out.append(np.asarray(packed)[at:at + s])
        at += s
    assert at == np.asarray(packed).size
    return out


def _abs_bank(bank):
    return tuple(np.abs(np.asarray(b, dtype=LD)) for b in bank)


def abs_wavedec(x, bank, level: int, mode: str):
    """Abs_l[i] per coefficient: the cascade of |taps| on |values|"""
    return wavedec(np.abs(np.asarray(x, dtype=LD)), _abs_bank(bank), level, mode)


def abs_waverec(coeffs, bank, mode: str, signal_len: int):
    """the synthesis cascade of |taps| on |coefficients|, per reconstructed sample"""
    return waverec([np.abs(np.asarray(c, dtype=LD)) for c in coeffs], _abs_bank(bank), mode, signal_len)


def legall53():
    """the LeGall 5/3 pair, zero-padded to F = 6 in PyWavelets' layout (bior2.2): rec is not dec reversed"""
    s = np.sqrt(LD(2))
    dec_lo = np.array([0, -1, 2, 6, 2, -1], dtype=LD) * s / 8
    dec_hi = np.array([0, 2, -4, 2, 0, 0], dtype=LD) * s / 8
    rec_lo = np.array([0, 2, 4, 2, 0, 0], dtype=LD) * s / 8
    rec_hi = np.array([0, 1, 2, -6, 2, 1], dtype=LD) * s / 8
    return dec_lo, dec_hi, rec_lo, rec_hi
