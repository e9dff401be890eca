"""Plain NumPy statement of one optimizer step, for the fused-optimizer tests (tests/test_optim_cpu.py pins it to
``torch.optim`` in float64; tests/test_optim_gpu.py holds ``lf_adam_step`` / ``lf_sgd_step`` / ``lf_rmsprop_step`` to it).

``adam_step`` / ``sgd_step`` / ``rmsprop_step`` are the arithmetic of ``torch.optim.Adam``, ``SGD(momentum, dampening 0, no
Nesterov)`` and ``RMSprop(momentum, not centred)`` on fp64 arrays: L2 weight decay folded into the gradient, Adam's first moment
as a lerp, ``eps`` added after the square root.  ``step_f32`` evaluates the same formulas unfused with every operation rounded to
fp32 (the order of ``torch.optim``'s own loops): it is the honest-fp32 yardstick that sizes ``tolerance``.

``tolerance`` is a forward rounding bound with u = 2**-24: per output, K*u times the sum of the absolute values of the terms that
enter it, the moments' bounds carried into the parameter through the update formula (the second moment's at half weight through
the square root).  K is the smallest power of two for which ``step_f32`` stays within HALF the bound on the value tests' inputs
(tests/test_optim_cpu.py asserts that, and that the wrong variants of the formulas leave the bound on the same inputs).

The scalars reach the kernels through a C ABI of ``float`` arguments, so the operation a launch is asked to perform has the
fp32-rounded settings; ``hyper`` returns those values (as Python floats) and the one-step tests hand the SAME values to the
reference.  That is not a loosening: e.g. Adam's beta2 = 0.999 is 0.99900001287 as a float, and a step that decays with one and
corrects the bias with the other is off by 1.3e-5 in ``1 - beta2`` -- 200 u.  The drift test, which compares with torch over a
run, gives the reference the unrounded settings.
"""
import numpy as np

U = 2.0 ** -24
K = 8

KINDS = ("adam", "sgd", "rmsprop")
# module order of the value tests' layout: running element offsets put the tensors with a full 4096-element chunk at flat-buffer
# offsets of every residue mod 4 (tests/test_optim_gpu.py asserts the residues)
SIZES = (4096, 1, 4097, 8192, 3, 255, 1023, 8191, 4095, 256, 12289)
LR = 1e-3
# (kind, weight_decay, grad_scale, Adam's 1-based step or None)
VALUE_CASES = tuple((kind, wd, gs, k) for kind in KINDS for wd in (0.0, 1e-2) for gs in (1.0, 0.125)
                    for k in ((1, 2, 7, 1000) if kind == "adam" else (None,)))


def f32(x):
    return float(np.float32(x))


def hyper(kind, lr, weight_decay, rounded=True):
    """The settings ``define_optim(kind, params, lr, weight_decay)`` builds, as the kernel receives them (``rounded``)."""
    r = f32 if rounded else float
    if kind == "adam":
        return dict(lr=r(lr), b1=r(0.9), b2=r(0.999), eps=r(1e-8), wd=r(weight_decay))
    if kind == "sgd":
        return dict(lr=r(lr), momentum=r(0.9), wd=r(weight_decay))
    if kind == "rmsprop":
        return dict(lr=r(lr), alpha=r(0.99), eps=r(1e-8), momentum=r(0.9), wd=r(weight_decay))
    raise KeyError(kind)


def make_inputs(seed, sizes=SIZES):
    """Per tensor fp32 arrays p, g, m, v where an optimizer goes wrong: g, m, sqrt(v) = sign * 10**U(-10, 2) per element (so
    sqrt(v) crosses eps = 1e-8 and the terms of every sum differ by up to twelve decades), p = sign * 10**U(-3, 1), and a block
    of exact zeros in g, m, v (0 / (0 + eps) is 0, not NaN)."""
    rng = np.random.default_rng(seed)

    def logu(n, lo, hi):
        return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)).astype(np.float32)
    out = []
    for n in sizes:
        p, g, m, s = logu(n, -3, 1), logu(n, -10, 2), logu(n, -10, 2), logu(n, -10, 2)
        v = s * s
        if n >= 3:
            z = slice(n // 3, n // 3 + max(1, n // 16))
            g[z] = m[z] = v[z] = 0
        out.append(dict(p=p, g=g, m=m, v=v))
    return out


def _grad(p, g, wd, grad_scale):
    g = grad_scale * g
    return g + wd * p if wd != 0 else g


def adam_step(p, g, m, v, lr, b1, b2, eps, wd, grad_scale, step):
    """One ``torch.optim.Adam`` step (1-based ``step``) -> p, exp_avg, exp_avg_sq."""
    g = _grad(p, g, wd, grad_scale)
    m = m + (1 - b1) * (g - m)
    v = b2 * v + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    return p - lr / bc1 * m / (np.sqrt(v) / np.sqrt(bc2) + eps), m, v


def sgd_step(p, g, m, v, lr, momentum, wd, grad_scale):
    """One ``torch.optim.SGD(momentum)`` step -> p, momentum_buffer, v (untouched: SGD has no second moment)."""
    m = momentum * m + _grad(p, g, wd, grad_scale)
    return p - lr * m, m, v


def rmsprop_step(p, g, m, v, lr, alpha, eps, momentum, wd, grad_scale):
    """One ``torch.optim.RMSprop(momentum)`` step -> p, momentum_buffer, square_avg."""
    g = _grad(p, g, wd, grad_scale)
    v = alpha * v + (1 - alpha) * g * g
    m = momentum * m + g / (np.sqrt(v) + eps)
    return p - lr * m, m, v


def step_f64(kind, p, g, m, v, hp, grad_scale=1.0, step=None):
    """One step of ``kind`` on fp64 copies of the inputs -> p, first-moment-like buffer, second-moment-like buffer."""
    f = np.float64
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    if kind == "adam":
        return adam_step(p, g, m, v, grad_scale=grad_scale, step=step, **hp)
    return (sgd_step if kind == "sgd" else rmsprop_step)(p, g, m, v, grad_scale=grad_scale, **hp)


def step_f32(kind, p, g, m, v, hp, grad_scale=1.0, step=None):
    """The same step unfused in fp32: every operation rounds, in the order of torch.optim's own (single-tensor) loops; the scalar
    factors are formed in double and rounded once, as a scalar handed to a tensor operation is."""
    f = np.float32
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    g = g * f(grad_scale)
    if hp["wd"] != 0:
        g = g + f(hp["wd"]) * p
    if kind == "adam":
        b1, b2 = hp["b1"], hp["b2"]
        m = m + f(1 - b1) * (g - m)
        v = v * f(b2) + f(1 - b2) * g * g
        denom = np.sqrt(v) / f(np.sqrt(1 - b2 ** step)) + f(hp["eps"])
        return p + f(-hp["lr"] / (1 - b1 ** step)) * (m / denom), m, v
    if kind == "sgd":
        m = m * f(hp["momentum"]) + g
        return p + f(-hp["lr"]) * m, m, v
    v = v * f(hp["alpha"]) + f(1 - hp["alpha"]) * g * g
    m = m * f(hp["momentum"]) + g / (np.sqrt(v) + f(hp["eps"]))
    return p + f(-hp["lr"]) * m, m, v


def tolerance(kind, p, g, m, v, hp, grad_scale=1.0, step=None):
    """Per-element bounds (tp, tm, tv) on |fp32 result - fp64 result| of one step from these inputs.  A = |grad_scale g| + wd |p|
    bounds the effective gradient term by term (so a cancelling sum keeps its absolute error), A**2 its square."""
    f = np.float64
    p, g, m, v = (np.asarray(a, f) for a in (p, g, m, v))
    ku = K * U
    wd, lr = hp["wd"], hp["lr"]
    A = np.abs(grad_scale * g) + wd * np.abs(p)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == "sgd":
            pn, mn, _ = sgd_step(p, g, m, v, grad_scale=grad_scale, **hp)
            tm = ku * (np.abs(m) + A)
            return U * np.abs(pn) + ku * lr * np.abs(mn) + lr * tm, tm, np.zeros_like(v)
        tv = ku * (np.abs(v) + A * A)
        if kind == "adam":
            pn, mn, vn = adam_step(p, g, m, v, grad_scale=grad_scale, step=step, **hp)
            bc1, bc2 = 1 - hp["b1"] ** step, 1 - hp["b2"] ** step
            root = np.sqrt(vn) / np.sqrt(bc2)
            denom = root + hp["eps"]
            upd = lr / bc1 * mn / denom
            half_rel_v = np.where(vn > 0, 0.5 * tv / vn, 0.0)
            tm = ku * (np.abs(m) + A)
            tp = U * np.abs(pn) + ku * np.abs(upd) + lr / bc1 * tm / denom + np.abs(upd) * half_rel_v * root / denom
            return tp, tm, tv
        pn, mn, vn = rmsprop_step(p, g, m, v, grad_scale=grad_scale, **hp)
        root = np.sqrt(vn)
        denom = root + hp["eps"]
        r = np.abs(_grad(p, g, wd, grad_scale)) / denom
        half_rel_v = np.where(vn > 0, 0.5 * tv / vn, 0.0)
        tm = ku * (np.abs(m) + r) + ku * A / denom + r * half_rel_v * root / denom
        return U * np.abs(pn) + ku * lr * np.abs(mn) + lr * tm, tm, tv
