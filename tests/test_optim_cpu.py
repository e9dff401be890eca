"""The fused-optimizer tests' reference and bound, pinned without a GPU (tests/optim_ref.py; the kernels are held to them in
tests/test_optim_gpu.py).

* the fp64 reference IS ``torch.optim.Adam`` / ``SGD`` / ``RMSprop`` as the upstream ``define_optim`` builds them: ten float64
  steps on the CPU, per element to 1e-13, a tensor that starts late included;
* the bound holds for honest fp32: the unfused fp32 evaluation of the same formulas, on the value tests' inputs, stays within
  half of ``tolerance`` for both moments.  The parameter's bound opens with ``u |p_new|``, the final rounding of ``p - update``,
  which no factor scales: a correctly rounded subtraction reaches it (observed 0.98 - 1.00 in every case) and nothing can exceed
  it, so for the parameter the half applies to the rest of the bound -- error <= u |p_new| + (tp - u |p_new|) / 2.
  Largest observed ratios over the 24 value cases at K = 8 (m and v: error / bound; p: (error - u |p_new|) / (tp - u |p_new|)):
      adam     p 0.19   m 0.13   v 0.24
      sgd      p 0.14   m 0.34   v -
      rmsprop  p 0.12   m 0.23   v 0.24
  K = 4 doubles them and SGD's momentum buffer leaves the half (0.67), so K = 8 is the smallest power of two;
* the bound is sharp: the fp64 reference evaluated WRONGLY leaves it on the same inputs.  Observed smallest share of violating
  elements over the cases each variant applies to (asserted floor in brackets):
      adam, eps under the square root         45 %  [25 %]
      adam, bias correction one step behind   63 %  [25 %]
      adam, lerp weight b1                    94 %  [1 %]
      weight decay omitted                    94 %  [1 %]
      weight decay on p (AdamW style)         96 %  [1 %]
      grad_scale omitted                      74 %  [1 %]
      rmsprop, eps under the square root      49 %  [1 %]
      sgd, dampening 1 - momentum             80 %  [1 %]
"""
import numpy as np
import pytest
import torch

import optim_ref as R


def _torch_optimizer(kind, params, lr, wd):
    """What the upstream project's define_optim returns."""
    if kind == "adam":
        return torch.optim.Adam(params, lr=lr, weight_decay=wd)
    if kind == "sgd":
        return torch.optim.SGD(params, lr=lr, momentum=0.9, weight_decay=wd)
    return torch.optim.RMSprop(params, lr=lr, momentum=0.9, weight_decay=wd)


_STATE = {"adam": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer", None), "rmsprop": ("momentum_buffer", "square_avg")}


@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_is_torch_float64(kind, wd):
    rng = np.random.default_rng(3)
    sizes, late, start, lr = [7, 33, 5], 2, 4, 1e-2
    hp = R.hyper(kind, lr, wd, rounded=False)
    par = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n))) for n in sizes]
    opt = _torch_optimizer(kind, par, lr, wd)
    ref = [dict(p=p.detach().numpy().copy(), m=np.zeros(n), v=np.zeros(n), k=0) for p, n in zip(par, sizes)]
    worst = 0.0
    for it in range(10):
        for i, (p, r) in enumerate(zip(par, ref)):
            if i == late and it < start:
                continue
            g = rng.standard_normal(p.numel())
            p.grad = torch.from_numpy(g.copy())
            r["k"] += 1
            r["p"], r["m"], r["v"] = R.step_f64(kind, r["p"], g, r["m"], r["v"], hp, 1.0, r["k"])
        opt.step()
        for i, (p, r) in enumerate(zip(par, ref)):
            if not r["k"]:
                assert not opt.state[p] and np.array_equal(p.detach().numpy(), r["p"])
                continue
            st = opt.state[p]
            assert int(st.get("step", r["k"])) == r["k"]
            for got, want in [(p.detach(), r["p"]), (st[_STATE[kind][0]], r["m"])] + (
                    [(st[_STATE[kind][1]], r["v"])] if _STATE[kind][1] else []):
                rel = np.abs(got.numpy() - want) / np.abs(want)
                worst = max(worst, float(rel.max()))
                assert (rel <= 1e-13).all(), (kind, wd, it, i)
    assert ref[late]["k"] == 10 - start
    print("%s wd=%g: reference vs torch.optim in float64, largest relative difference %.1e" % (kind, wd, worst))


@pytest.fixture(scope="module")
def inputs():
    cat = {k: np.concatenate([t[k] for t in R.make_inputs(0)]) for k in "pgmv"}
    for a in cat.values():
        a.setflags(write=False)
    return cat


def _cases(kind):
    return [c for c in R.VALUE_CASES if c[0] == kind]


@pytest.mark.parametrize("kind", R.KINDS)
def test_bound_holds_for_unfused_fp32(kind, inputs):
    worst = dict(p=0.0, m=0.0, v=0.0, p_whole=0.0)
    for _, wd, gs, k in _cases(kind):
        hp = R.hyper(kind, R.LR, wd)
        a = [inputs[n] for n in "pgmv"]
        want, got, tol = R.step_f64(kind, *a, hp, gs, k), R.step_f32(kind, *a, hp, gs, k), R.tolerance(kind, *a, hp, gs, k)
        assert all(x.dtype == np.float32 for x in got)
        err = [np.abs(x.astype(np.float64) - w) for x, w in zip(got, want)]
        last = R.U * np.abs(want[0])                       # the final rounding of p - update: at most this, and unscaled
        assert (err[0] <= last + 0.5 * (tol[0] - last)).all(), (kind, wd, gs, k)
        assert (err[1] <= 0.5 * tol[1]).all() and (err[2] <= 0.5 * tol[2]).all(), (kind, wd, gs, k)
        over = err[0] > last
        worst["p"] = max(worst["p"], float(((err[0] - last)[over] / (tol[0] - last)[over]).max(initial=0.0)))
        worst["p_whole"] = max(worst["p_whole"], float((err[0][err[0] > 0] / tol[0][err[0] > 0]).max()))
        for n, e, t in (("m", err[1], tol[1]), ("v", err[2], tol[2])):
            worst[n] = max(worst[n], float((e[e > 0] / t[e > 0]).max(initial=0.0)))
    print("%s: unfused fp32 / bound at K = %d: p %.2f (whole bound, final rounding included: %.2f)  m %.2f  v %.2f"
          % (kind, R.K, worst["p"], worst["p_whole"], worst["m"], worst["v"]))
    assert worst["p_whole"] <= 1.0


def _wrong(kind, how, p, g, m, v, hp, gs, k):
    """The fp64 formulas of optim_ref with ONE deliberate mistake."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    lr, wd = hp["lr"], hp["wd"]
    g = g if how == "no_grad_scale" else gs * g
    if how == "decoupled_wd":
        p = p * (1 - lr * wd)
    elif how != "no_wd":
        g = g + wd * p
    if kind == "adam":
        b1, b2, eps = hp["b1"], hp["b2"], hp["eps"]
        m = m + (b1 if how == "lerp_b1" else 1 - b1) * (g - m)
        v = b2 * v + (1 - b2) * g * g
        kk = k - 1 if how == "bias_behind" else k
        bc1, bc2 = 1 - b1 ** kk, 1 - b2 ** kk
        denom = np.sqrt(v + eps) / np.sqrt(bc2) if how == "eps_under_sqrt" else np.sqrt(v) / np.sqrt(bc2) + eps
        return p - lr / bc1 * m / denom, m, v
    if kind == "sgd":
        m = hp["momentum"] * m + ((1 - hp["momentum"]) if how == "dampening" else 1.0) * g
        return p - lr * m, m, v
    v = hp["alpha"] * v + (1 - hp["alpha"]) * g * g
    m = hp["momentum"] * m + g / (np.sqrt(v + hp["eps"]) if how == "eps_under_sqrt" else np.sqrt(v) + hp["eps"])
    return p - lr * m, m, v


# (name, kinds, which value cases, least share of elements that must leave the bound)
_VARIANTS = [
    ("eps_under_sqrt", ("adam",), lambda wd, gs, k: True, 0.25),
    ("bias_behind", ("adam",), lambda wd, gs, k: k >= 2, 0.25),
    ("lerp_b1", ("adam",), lambda wd, gs, k: True, 0.01),
    ("no_wd", R.KINDS, lambda wd, gs, k: wd != 0, 0.01),
    ("decoupled_wd", R.KINDS, lambda wd, gs, k: wd != 0, 0.01),
    ("no_grad_scale", R.KINDS, lambda wd, gs, k: gs != 1, 0.01),
    ("eps_under_sqrt", ("rmsprop",), lambda wd, gs, k: True, 0.01),
    ("dampening", ("sgd",), lambda wd, gs, k: True, 0.01),
]


@pytest.mark.parametrize("how,kinds,applies,floor", _VARIANTS, ids=["%s-%s" % (v[0], "+".join(v[1])) for v in _VARIANTS])
def test_bound_is_sharp(how, kinds, applies, floor, inputs):
    a = [inputs[n] for n in "pgmv"]
    least, n = 1.0, 0
    for kind, wd, gs, k in R.VALUE_CASES:
        if kind not in kinds or not applies(wd, gs, k):
            continue
        hp = R.hyper(kind, R.LR, wd)
        want, tol = R.step_f64(kind, *a, hp, gs, k), R.tolerance(kind, *a, hp, gs, k)
        got = _wrong(kind, how, *a, hp, gs, k)
        out = np.zeros(a[0].shape, bool)
        for x, w, t in zip(got, want, tol):
            out |= np.abs(x - w) > t
        share = float(out.mean())
        assert share >= floor, (how, kind, wd, gs, k, share)
        least, n = min(least, share), n + 1
    assert n
    print("%s (%s): leaves the bound on at least %.0f %% of the elements in each of %d cases" % (how, "+".join(kinds), 100 * least, n))
