"""Plain NumPy statement of ``torch.nn.utils.clip_grad_norm_`` (2-norm, ``error_if_nonfinite=False``) for the clipping tests:
tests/test_clip_grad_cpu.py pins it to torch on the CPU, tests/test_clip_grad_gpu.py holds ``lf_grad_sumsq`` /
``lf_grad_norm_finish`` / ``lf_grad_scale_inplace`` and the ``lf_*_step_clipped`` launches to it.

    total_norm = grad_scale * sqrt(sum over all tensors of g**2)
    coef       = max_norm / (total_norm + 1e-6), replaced by 1 where that exceeds 1 (a NaN stays a NaN: torch's clamp(max=1.0))
    g_clipped  = (g * grad_scale) * coef          -- two separately rounded products in the gradient's own format

``grad_scale`` is the optimizers' (1 / world size for summed data-parallel gradients); torch's routine has none, i.e. 1.
"""
import numpy as np

U = 2.0 ** -24
# |total_norm - fp64 norm| <= NORM_TOL * norm: an fp64 accumulation of <= 2**21 squares leaves ~1e-13, the ONE rounding of the
# result to fp32 leaves u = 2**-24; twice that.  (torch's own fp32 routine on the CPU sits at 1.4 u on the tests' inputs.)
NORM_TOL = 2 * U


def norm_f64(grads, grad_scale=1.0):
    """grad_scale * sqrt(sum g**2), every element widened to fp64 first."""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(grad_scale) * float(np.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads)))


def coef(total_norm, max_norm, dtype=np.float32):
    """The clip coefficient in ``dtype`` arithmetic from a norm already rounded to ``dtype``."""
    f = dtype
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = f(max_norm) / (f(total_norm) + f(1e-6))
    return f(1) if c > 1 else f(c)


def coef_as_torch_rounds_it(total_norm, max_norm, dtype=np.float32):
    """torch evaluates ``max_norm / tensor`` as ``tensor.reciprocal() * max_norm``: two roundings where ``coef`` has one, so the two
    differ by at most 3 units of the format's rounding error (2 of torch's, 1 of the quotient's)."""
    f = dtype
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        c = (f(1) / (f(total_norm) + f(1e-6))) * f(max_norm)
    return f(1) if c > 1 else f(c)


def effective(g, grad_scale, c):
    """The gradient the clipped step uses / the drop-in form leaves behind: fl(fl(g * grad_scale) * coef) in g's format."""
    g = np.asarray(g)
    f = g.dtype.type
    with np.errstate(over="ignore", invalid="ignore"):
        return (g * f(grad_scale)) * f(c)


def clip(grads, max_norm, grad_scale=1.0):
    """(total_norm, coef, clipped gradients) for a list of arrays of one float format."""
    f = np.asarray(grads[0]).dtype.type
    total = f(norm_f64(grads, grad_scale))
    c = coef(total, max_norm, f)
    return total, c, [effective(g, grad_scale, c) for g in grads]
