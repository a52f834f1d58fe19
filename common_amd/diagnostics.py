"""Convergence diagnostics of a scalar traced over several chains -- the log joint that chains.JointTracker records, an
hp coordinate of RunResult.values, a group count: split-R-hat and the effective sample size, on the host in numpy.
Needs neither the shared library nor a GPU.

Both take x [chains, samples] and split every chain into its first and its last floor(samples / 2) draws (an odd count
drops the middle draw), so that a chain that drifts disagrees with itself: m = 2 chains sequences of n = samples // 2.

  split_rhat   Gelman et al., Bayesian Data Analysis (3rd ed.), section 11.4, as Stan computes it:
                 W = the mean of the sequences' variances (ddof 1), B / n = the variance of their means (ddof 1),
                 var+ = (n - 1) / n W + B / n,  R-hat = sqrt(var+ / W)
  ess          BDA3 (11.8) with Geyer's (1992) truncation, as Stan computes it: per sequence the autocovariances
               acov_t = 1/n sum_i (x_i - mean)(x_{i+t} - mean) by FFT, the sequences' variances s2 = acov_0 n / (n - 1),
               W and var+ as above, the combined
                 rho_t = 1 - (W - mean over the sequences of acov_t) / var+
               Geyer's initial positive sequence -- pairs P_k = rho_{2k} + rho_{2k+1} are kept while they are positive --
               made monotone (a pair larger than the one before is replaced by it), and
                 tau = -1 + 2 sum of the kept rho_t (+ the first rho of the pair that ended the sequence, if positive),
                 ess = m n / tau,  tau held at or above 1 / log10(m n) (Stan's cap for antithetic chains).
Fewer than 4 samples, or no variance inside the sequences (W == 0), or a value that is not finite: nan.
"""
import numpy as np


def _split(x):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x must be [chains, samples]")
    if x.shape[0] < 1:
        raise ValueError("x must hold at least one chain")
    s = x.shape[1]
    if s < 4 or not np.all(np.isfinite(x)):
        return None
    n = s // 2
    return np.concatenate([x[:, :n], x[:, s - n:]], axis=0)


def split_rhat(x):
    """split-R-hat of x [chains, samples] (the module's docstring); nan for a degenerate input"""
    y = _split(x)
    if y is None:
        return float("nan")
    n = y.shape[1]
    w = float(np.mean(np.var(y, axis=1, ddof=1)))
    if not w > 0.0:
        return float("nan")
    b_over_n = float(np.var(np.mean(y, axis=1), ddof=1))
    return float(np.sqrt(((n - 1.0) / n * w + b_over_n) / w))


def autocovariance(y):
    """acov[j, t] = 1/n sum_i (y[j, i] - mean_j)(y[j, i + t] - mean_j) of every row of y, by FFT (zero-padded to twice
    the length, so the circular products are the linear ones)"""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[1]
    size = 1
    while size < 2 * n:
        size *= 2
    f = np.fft.rfft(y - y.mean(axis=1, keepdims=True), n=size, axis=1)
    return np.fft.irfft(f * np.conj(f), n=size, axis=1)[:, :n] / n


def ess(x):
    """effective sample size of x [chains, samples] over all chains (the module's docstring); nan for a degenerate
    input"""
    y = _split(x)
    if y is None:
        return float("nan")
    m, n = y.shape
    acov = autocovariance(y)
    w = float(np.mean(acov[:, 0] * n / (n - 1.0)))
    if not w > 0.0:
        return float("nan")
    var_plus = w * (n - 1.0) / n + float(np.var(np.mean(y, axis=1), ddof=1))
    mean_acov = acov.mean(axis=0)

    def rho_at(t):
        return 1.0 - (w - mean_acov[t]) / var_plus if t < n else 0.0

    rho = np.zeros(n + 3)
    even, odd = 1.0, rho_at(1)
    rho[0], rho[1] = even, odd
    t = 1
    while t < n - 4 and even + odd > 0.0:
        even, odd = rho_at(t + 1), rho_at(t + 2)
        if even + odd >= 0.0:
            rho[t + 1], rho[t + 2] = even, odd
        t += 2
    max_t = t
    if even > 0.0:
        rho[max_t + 1] = even
    t = 1
    while t <= max_t - 3:                               # the pairs made monotone
        if rho[t + 1] + rho[t + 2] > rho[t - 1] + rho[t]:
            rho[t + 1] = 0.5 * (rho[t - 1] + rho[t])
            rho[t + 2] = rho[t + 1]
        t += 2
    tau = -1.0 + 2.0 * float(np.sum(rho[:max_t])) + float(rho[max_t + 1])
    tau = max(tau, 1.0 / np.log10(m * n))
    return float(m * n / tau)
