"""TEST INFRASTRUCTURE ONLY (the yardstick, never the product): the learners' Adam
step (k_adam in csrc/learner.hip, k_lc_adam in csrc/learner_common.h) restated
three times, the bar that follows from the three, and the step-by-step checker
that tests/test_learner_optimizer_gpu.py runs against the device and
tests/test_adam_ref_cpu.py against planted mistakes.

  adam64      float64, torch.optim.Adam's semantics (pinned to it in test_adam_ref_cpu.py)
  adam32      numpy float32 in the kernels' exact operation order: what the device
              must produce bit for bit (correctly rounded sqrtf and division, no
              contraction: the build passes -ffp-contract=off)
  adam32_alt  float32 in the algebraically equal "hat" order; only sizes the bar

Every setting is rounded to float32 first, because the device receives floats.
"""
import math

import numpy as np

DEFAULTS = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, bn_momentum=0.1, bn_eps=1e-5)
CONFIG_A = {}
CONFIG_B = dict(lr=3e-3, beta1=0.8, beta2=0.95, eps=1e-3, bn_momentum=0.3, bn_eps=1e-2)
CONFIG_C = dict(lr=0.0, beta1=0.0, beta2=0.5)   # trainable entries must not move; the running statistics still do
CONFIGS = dict(A=CONFIG_A, B=CONFIG_B, C=CONFIG_C)
TINY = 2.0 ** -126    # the smallest normal float32
MASK_LIMIT = 0.01     # at most this share of the trainable entries may sit in the subnormal mask
MARGIN = 4.0          # the project's margin over a reference-only spread


def settings(cfg):
    """DEFAULTS overlaid with cfg, every value as the float32 the device receives"""
    unknown = set(cfg) - set(DEFAULTS)
    assert not unknown, unknown
    return {k: float(np.float32(cfg.get(k, v))) for k, v in DEFAULTS.items()}


def restatement_kw(cfg):
    """cfg as the keyword arguments of the float64 restatements' train_step / train"""
    s = settings(cfg)
    return dict(lr=s["lr"], b1=s["beta1"], b2=s["beta2"], eps=s["eps"], momentum=s["bn_momentum"], bn_eps=s["bn_eps"])


def bias_corrections(t, cfg):
    """(1 - b1^t, sqrt(1 - b2^t)) in double, as the learners' host code computes them"""
    s = settings(cfg)
    return 1.0 - math.pow(s["beta1"], float(t)), math.sqrt(1.0 - math.pow(s["beta2"], float(t)))


def adam64(p, g, m, v, t, cfg):
    """step t (1-based) in float64; returns (p, m, v)"""
    s = settings(cfg)
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = s["beta1"], s["beta2"]
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - s["lr"] / (1 - b1 ** t) * m / (np.sqrt(v) / math.sqrt(1 - b2 ** t) + s["eps"])
    return p, m, v


def _f32_settings(t, cfg):
    s = settings(cfg)
    bc1, bc2 = bias_corrections(t, cfg)
    f = np.float32
    return f(s["lr"]), f(s["beta1"]), f(s["beta2"]), f(s["eps"]), f(bc1), f(bc2)


def adam32(p, g, m, v, t, cfg):
    """step t in float32, the kernels' operation order:
        mi = b1 * m + (1.0f - b1) * g;  vi = b2 * v + (1.0f - b2) * g * g   (left to right)
        p -= (lr / bc1) * (mi / (sqrtf(vi) / bc2 + eps))
    returns (p, m, v, mask): mask marks the entries where some intermediate is
    non-zero and below 2^-126 (tested in float64), where a device that treats
    subnormals differently in sqrt or division may legitimately differ."""
    lr, b1, b2, eps, bc1, bc2 = _f32_settings(t, cfg)
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    one = np.float32(1.0)
    omb1, omb2 = one - b1, one - b2
    with np.errstate(under="ignore", invalid="ignore", divide="ignore"):
        a1, a2 = b1 * m, omb1 * g
        mi = a1 + a2
        c1, c2 = b2 * v, omb2 * g
        c3 = c2 * g
        vi = c1 + c3
        r = np.sqrt(vi)
        q = r / bc2
        den = q + eps
        w = mi / den
        k = lr / bc1
        upd = k * w
        out = p - upd
        d = np.float64
        exact = [d(b1) * d(m), d(omb1) * d(g), d(a1) + d(a2), d(b2) * d(v), d(omb2) * d(g), d(c2) * d(g), d(c1) + d(c3),
                 np.sqrt(d(vi)), d(r) / d(bc2), d(q) + d(eps), d(mi) / d(den), d(k) * d(w)]
    mask = np.zeros(p.shape, bool)
    for e in exact:
        mask |= (e != 0) & (np.abs(e) < TINY)
    for a in (mi, vi, out):
        assert a.dtype == np.float32
    return out, mi, vi, mask


def adam32_alt(p, g, m, v, t, cfg):
    """the "hat" form lr * ((m / bc1) / (sqrt(v / bc2^2) + eps)) in float32; returns (p, m, v)"""
    lr, b1, b2, eps, bc1, bc2 = _f32_settings(t, cfg)
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    one = np.float32(1.0)
    with np.errstate(under="ignore", invalid="ignore", divide="ignore"):
        mi = b1 * m + (one - b1) * g
        vi = b2 * v + (one - b2) * g * g
        out = p - lr * ((mi / bc1) / (np.sqrt(vi / (bc2 * bc2)) + eps))
    return out, mi, vi


def ulp32(x):
    """the spacing of float32 at |x|"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def bar(p_prev, p_new, spread):
    """per entry: 1 ulp32(max(|p_prev|, |p_new|)) + 4 x spread"""
    big = np.maximum(np.abs(np.asarray(p_prev, np.float64)), np.abs(np.asarray(p_new, np.float64)))
    return ulp32(big) + MARGIN * spread


def _same_bits(a, b):
    return np.asarray(a, np.float32).view(np.uint32) == np.asarray(b, np.float32).view(np.uint32)


def adam_steps_report(read_step, p0, trainable, cfg, K):
    """Runs K steps through read_step(k) -> (G, P) (k = 1..K: one step of the thing
    under test, its gradient and its parameters afterwards, float32) and the three
    references beside it.  The references start every step from the tested side's
    previous parameters and carry their own moments, fed with its gradient.

    Returns a dict: spread (the largest distance between the three references on
    the update term p_prev - p_new over the trainable entries and all steps: from
    the references alone), and per step k the lists
      tier1[k-1]   max over the trainable entries of |P - adam64| / bar
      tier2[k-1]   number of trainable entries outside the subnormal mask where P != adam32 (bits)
      tier3[k-1]   number of trainable entries with G == 0 and zero moments that moved
      idle[k-1]    number of trainable entries with G == 0 and zero moments
      running[k-1] number of running-statistic entries with G != 0
      masked[k-1]  share of the trainable entries in the subnormal mask
      bc1[k-1]     float32(1 - b1^k)"""
    tr = np.asarray(trainable, bool)
    p0 = np.asarray(p0, np.float32).copy()
    n = p0.size
    record = []
    for k in range(1, K + 1):
        G, P = read_step(k)
        G, P = np.asarray(G, np.float32).copy(), np.asarray(P, np.float32).copy()
        assert G.shape == P.shape == (n,)
        record.append((G, P))

    def references():
        """per step: the three references from the recorded gradients and parameters"""
        p_prev = p0
        m64 = v64 = np.zeros(n)
        m32 = v32 = ma = va = np.zeros(n, np.float32)
        for k, (G, P) in enumerate(record, 1):
            idle = (G == 0) & (m32 == 0) & (v32 == 0)
            p64, m64, v64 = adam64(p_prev, G, m64, v64, k, cfg)
            p32, m32, v32, mask = adam32(p_prev, G, m32, v32, k, cfg)
            pa, ma, va = adam32_alt(p_prev, G, ma, va, k, cfg)
            yield dict(k=k, G=G, P=P, prev=p_prev, p64=p64, p32=p32, pa=pa, mask=mask, idle=idle)
            p_prev = P

    spread = 0.0   # first pass: the references alone
    for s in references():
        prev64 = s["prev"].astype(np.float64)
        u64, u32, ua = prev64 - s["p64"], prev64 - s["p32"], prev64 - s["pa"]
        for x, y in ((u32, u64), (ua, u64), (u32, ua)):
            spread = max(spread, float(np.abs(x - y)[tr].max()))
    rep = dict(spread=spread, tier1=[], tier2=[], tier3=[], idle=[], running=[], masked=[], bc1=[], cfg=settings(cfg),
               n_trainable=int(tr.sum()))
    for s in references():
        b = bar(s["prev"], s["p64"], spread)
        rep["tier1"].append(float((np.abs(s["P"].astype(np.float64) - s["p64"]) / b)[tr].max()))
        rep["tier2"].append(int((~_same_bits(s["P"], s["p32"]) & tr & ~s["mask"]).sum()))
        rep["tier3"].append(int((~_same_bits(s["P"], s["prev"]) & tr & s["idle"]).sum()))
        rep["idle"].append(int((s["idle"] & tr).sum()))
        rep["running"].append(int((s["G"][~tr] != 0).sum()))
        rep["masked"].append(float((s["mask"] & tr).sum()) / max(1, rep["n_trainable"]))
        rep["bc1"].append(_f32_settings(s["k"], cfg)[4])
    rep["moved"] = float(np.abs(record[-1][1].astype(np.float64) - p0)[tr].max())
    return rep


def assert_adam_report(rep, tier2=True):
    """the checks of check_adam_steps on a report"""
    worst = max(rep["masked"])
    assert worst <= MASK_LIMIT, "subnormal mask holds %.3g of the trainable entries (limit %g)" % (worst, MASK_LIMIT)
    assert not any(rep["running"]), "running statistics with a non-zero gradient: %s" % rep["running"]
    assert max(rep["tier1"]) <= 1.0, "tier 1: |P - adam64| is %.3g x the bar (spread %.3g), per step %s" % (
        max(rep["tier1"]), rep["spread"], ["%.3g" % x for x in rep["tier1"]])
    if tier2:
        assert not any(rep["tier2"]), "tier 2: entries that differ from adam32 in bits, per step %s" % rep["tier2"]
    assert not any(rep["tier3"]), "tier 3: idle entries (G == 0, zero moments) that moved, per step %s" % rep["tier3"]


def check_adam_steps(read_step, p0, trainable, cfg, K, tier2=True):
    """For steps k = 1..K, on the trainable entries: |P - adam64| <= bar everywhere;
    P == adam32 bit for bit outside the subnormal mask; entries with G == 0 and zero
    moments keep P_prev's bits.  On the running statistics: G == 0 exactly.  The
    subnormal mask may hold at most 1 % of the trainable entries at any step.
    Returns the report (adam_steps_report)."""
    rep = adam_steps_report(read_step, p0, trainable, cfg, K)
    print("adam steps: %s, K %d, spread %.3g, tier 1 worst %.3g x the bar, tier 2 mismatches %d, masked <= %.3g" % (
        {k: float(np.float32(v)) for k, v in cfg.items()} or "defaults", K, rep["spread"], max(rep["tier1"]), sum(rep["tier2"]), max(rep["masked"])))
    assert_adam_report(rep, tier2)
    return rep


def trainable_mask(convs, n):
    """everything but the BatchNorm running statistics (convs: a restatement's _layout()[0])"""
    tr = np.ones(n, bool)
    for c in convs:
        tr[c["mu"]:c["mu"] + c["co"]] = False
        tr[c["var"]:c["var"] + c["co"]] = False
    return tr
