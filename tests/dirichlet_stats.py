"""check_draws: is an [N][n] float32 array N draws of Dirichlet(alpha, ..., alpha)?

The yardstick of the root-noise sampler (csrc/dirichlet.h) in
tests/test_chess_root_noise_gpu.py; tests/test_chess_root_noise_cpu.py shows on
numpy's own sampler that it passes correct draws and catches the mistakes a
Gamma-based sampler can make.  Every bound comes from the exact distribution:

  rows       finite, >= 0, |sum - 1| <= n * 2^-23 (each component carries at most
             half a float32 ulp of its own size, the normalising sum a few more)
  means      component j's mean over N draws is 1/n with the exact variance
             (n - 1) / (n^2 (n alpha + 1)) / N; max_j |z_j| <= 5
  variance   the mean over components of sample variance / exact variance lies
             in [0.95, 1.05]
  marginals  components 0, n - 1 and (n > 64) 64 -- the first lane, the last child
             and the second pass of a wave -- against Beta(alpha, (n - 1) alpha),
             Kolmogorov-Smirnov p >= 1e-4 each

GRID leaves out n = 2 with alpha < 1: float32 rounds a visible share of Beta(0.1,
0.1) to exactly 1.0, and numpy's draws cast to float32 fail the marginal test there.
"""
import numpy as np
from scipy import stats

GRID = [(2, 1.0), (2, 3.0), (20, 0.1), (20, 0.3), (20, 1.0), (65, 0.3), (65, 3.0), (218, 0.1), (218, 0.3),
        (218, 1.0)]
N_DRAWS = 20000
Z_MAX, VAR_LO, VAR_HI, KS_P = 5.0, 0.95, 1.05, 1e-4


def exact_variance(n, alpha):
    return (n - 1.0) / (n * n * (n * alpha + 1.0))


def measure(eta, alpha):
    """the figures check_draws asserts on, as a dict"""
    eta = np.asarray(eta)
    assert eta.ndim == 2 and eta.dtype == np.float32, (eta.shape, eta.dtype)
    N, n = eta.shape
    x = eta.astype(np.float64)
    out = dict(N=N, n=n, alpha=alpha, finite=bool(np.isfinite(x).all()), min=float(x.min()),
               sum_err=float(np.abs(x.sum(1) - 1.0).max()), sum_bound=n * 2.0 ** -23)
    if n == 1:
        return out
    var = exact_variance(n, alpha)
    z = (x.mean(0) - 1.0 / n) / np.sqrt(var / N)
    out["z_max"] = float(np.abs(z).max())
    out["var_ratio"] = float((x.var(0, ddof=1) / var).mean())
    comps = [0, n - 1] + ([64] if n > 64 else [])
    out["ks_p"] = {j: float(stats.kstest(x[:, j], stats.beta(alpha, (n - 1) * alpha).cdf).pvalue) for j in comps}
    return out


def check_draws(eta, alpha):
    """AssertionError unless eta [N][n] float32 looks like N draws of Dirichlet(alpha); returns the figures"""
    m = measure(eta, alpha)
    assert m["finite"], "non-finite component"
    assert m["min"] >= 0.0, m["min"]
    assert m["sum_err"] <= m["sum_bound"], ("row sum", m["sum_err"], m["sum_bound"])
    if m["n"] == 1:
        return m
    assert m["z_max"] <= Z_MAX, ("component mean", m["z_max"])
    assert VAR_LO <= m["var_ratio"] <= VAR_HI, ("pooled variance ratio", m["var_ratio"])
    for j, p in m["ks_p"].items():
        assert p >= KS_P, ("marginal of component", j, p)
    return m
