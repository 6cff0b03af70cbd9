"""Float64 numpy restatement of the true-peak measurement (csrc/truepeak.hip, include/p2phd.h): the polyphase table, the
oversampled magnitudes, the peak and the gain rule, exactly as the header defines them -- nothing of the library is used."""
import numpy as np


def bessel_i0(x):
    """I0(x), x >= 0: the power series, summed until a term no longer changes the sum."""
    q = 0.25 * float(x) * float(x)
    term = total = 1.0
    for m in range(1, 1000):
        term *= q / (m * m)
        if total + term == total:
            break
        total += term
    return total


def table(factor, taps_per_phase, beta):
    """c[F][P] in float64: c[p][k] = sinc(tau) I0(beta sqrt(1 - (tau / (P/2))^2)) / I0(beta), tau = (k - (P/2 - 1)) - p / F, every
    phase divided by its own sum; phase 0 the unit impulse at k = P/2 - 1."""
    F, P = int(factor), int(taps_per_phase)
    c = np.zeros((F, P), dtype=np.float64)
    c[0, P // 2 - 1] = 1.0
    i0b = bessel_i0(beta)
    for p in range(1, F):
        for k in range(P):
            tau = (k - (P // 2 - 1)) - p / F
            r = tau / (P // 2)
            c[p, k] = np.sinc(tau) * bessel_i0(beta * np.sqrt(max(0.0, 1.0 - r * r))) / i0b
        c[p] /= c[p].sum()
    return c


def clean(x):
    """x~ of the header: float64, every NaN or infinite sample taken as 0."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isfinite(x), x, 0.0)


def _windows(row, P):
    """[L + 1, P]: line i + 1 holds x~[i + k - (P/2 - 1)], k = 0 .. P - 1, for i = -1 .. L - 1; zeros outside the row."""
    L, h = len(row), P // 2 - 1
    ext = np.concatenate([np.zeros(h + 1), row, np.zeros(P)])                # ext[n + h + 1] = x~[n]
    return np.lib.stride_tricks.sliding_window_view(ext, P)[:L + 1]


def oversampled(x, c):
    """x [L], c [F][P] -> y [L + 1, F]: line i + 1 holds y[i][p] for i = -1 .. L - 1; column 0 is x~[i] itself (0 at i = -1),
    columns p >= 1 the sums over the table's phase p."""
    c = np.asarray(c, dtype=np.float64)
    row = clean(x)
    y = _windows(row, c.shape[1]) @ c.T
    y[:, 0] = np.concatenate([[0.0], row])
    return y


def abs_sums(x, c):
    """sum_k |c[p][k] x~[.]| for every y of `oversampled` with p >= 1 -> [L + 1, F - 1] (empty for F = 1): what the worst-case
    bound of an fp32 dot product multiplies."""
    c = np.asarray(c, dtype=np.float64)
    return np.abs(_windows(clean(x), c.shape[1])) @ np.abs(c[1:]).T


def true_peak(x, c):
    """Rows x [C, L] (or one row [L]) -> the true peak per row, float64."""
    x = np.asarray(x)
    if x.ndim == 1:
        return float(np.abs(oversampled(x, c)).max())
    return np.array([np.abs(oversampled(r, c)).max() for r in x], dtype=np.float64)


def dot_bound(x, c):
    """P 2^-24 max_p sum_k |c x| over every y of the rows x [C, L] -> one number per row: how far an fp32 true peak may lie from
    the float64 one (a maximum moves by no more than its largest operand's error)."""
    x = np.atleast_2d(np.asarray(x))
    P = np.asarray(c).shape[1]
    return np.array([P * 2.0 ** -24 * (abs_sums(r, c).max() if np.asarray(c).shape[0] > 1 else 0.0) for r in x], dtype=np.float64)


def gain(tpeaks, ceiling):
    """The gain rule in fp32: m > ceiling ? ceiling / m : 1 with m the largest true peak -- one fp32 division."""
    m = np.float32(np.max(np.asarray(tpeaks, dtype=np.float32))) if np.size(tpeaks) else np.float32(0.0)
    ceiling = np.float32(ceiling)
    return ceiling / m if m > ceiling else np.float32(1.0)


def ramped_tone(f, phi, n=9600, ramp=2400, amplitude=1.0):
    """amplitude sin(2 pi f n + phi) under raised-cosine ramps of `ramp` samples at both ends, float64 (an abrupt start has real
    overshoot of its own)."""
    t = np.arange(n, dtype=np.float64)
    env = np.ones(n)
    up = 0.5 - 0.5 * np.cos(np.pi * (np.arange(ramp) + 0.5) / ramp)
    env[:ramp], env[n - ramp:] = up, up[::-1]
    return amplitude * env * np.sin(2.0 * np.pi * f * t + phi)
