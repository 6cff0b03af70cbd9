"""Float64 numpy restatement of the time-domain crossover (include/p2phd.h: p2phd_xover_taps_fill, p2phd_xover_fwd;
generate.crossover_plan).  The reference has no such stage: this file is the specification the kernels are tested against."""
import numpy as np

BETA = 8.96
MAX_TAPS = 4095


def taps_ref(taps, cutoff, beta):
    """h[k] = 2 fc sinc(2 fc n) I0(beta sqrt(1 - (2 n / (taps - 1))^2)) / I0(beta), n = k - (taps - 1) / 2, over its sum; float64."""
    if taps == 1:
        return np.ones(1)
    n = np.arange(taps, dtype=np.float64) - (taps - 1) // 2
    r = 2.0 * n / (taps - 1)
    h = 2.0 * cutoff * np.sinc(2.0 * cutoff * n) * np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / np.i0(beta)
    return h / h.sum()


def diff_ref(sr, lr, level):
    """d = level * lr - sr in float64, [C, L]."""
    return np.float64(level) * np.asarray(lr, dtype=np.float64) - np.asarray(sr, dtype=np.float64)


def xover_ref(sr, lr, level, h):
    """out[c][i] = sr[c][i] + sum_k h[k] d[c][i + c0 - k], d zero-extended beyond [0, L), c0 = (taps - 1) / 2; float64, [C, L]."""
    sr = np.asarray(sr, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    d = diff_ref(sr, lr, level)
    c0 = (len(h) - 1) // 2
    out = np.empty_like(sr)
    for c in range(sr.shape[0]):
        out[c] = sr[c] + np.convolve(d[c], h, mode="full")[c0:c0 + sr.shape[1]]     # full[m] = sum_k h[k] d[m - k], m = i + c0
    return out


def abs_conv_ref(sr, lr, level, h):
    """(|h| (*) (|level| |lr| + |sr|))[i], the magnitude sum behind the float bound; [C, L]."""
    sr = np.abs(np.asarray(sr, dtype=np.float64))
    a = abs(float(level)) * np.abs(np.asarray(lr, dtype=np.float64)) + sr
    h = np.abs(np.asarray(h, dtype=np.float64))
    c0 = (len(h) - 1) // 2
    return np.stack([np.convolve(a[c], h, mode="full")[c0:c0 + sr.shape[1]] for c in range(sr.shape[0])])


def width_ref(hr_rate, taps):
    return (90.0 - 7.95) * hr_rate / (14.36 * (taps - 1))


def crossover_plan_ref(hr_rate, lr_rate, crossover_hz=None):
    """(taps, cutoff, beta) of the default plan: the smallest odd N >= 3 with crossover_hz + width(N) / 2 <= lr_rate / 2, by search."""
    fc = 0.95 * lr_rate / 2.0 if crossover_hz is None else float(crossover_hz)
    for n in range(3, 1 << 20, 2):
        if fc + width_ref(hr_rate, n) / 2.0 <= lr_rate / 2.0:
            return n, fc / hr_rate, BETA
    raise AssertionError("no plan")
