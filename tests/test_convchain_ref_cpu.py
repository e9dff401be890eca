"""tests/convchain_ref.py against torch's own autograd and modules, in fp64 on the CPU: the reference the GPU chain tests
(tests/test_convchain_shapes_gpu.py) compare with has to be right by itself."""
import pytest
import torch

import convchain_ref as R

CHAINS = [((16, 48, 64, 16), (3, 3, 3)), ((32, 16, 16), (1, 3)), ((16, 16), (3,))]
SHAPES = [(3, 6, 20), (2, 1, 16), (1, 3, 6)]


def make(channels, ksize, shape, seed):
    gen = torch.Generator().manual_seed(seed)
    N, H, W = shape
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    params, running = [], []
    for ci, co, k in zip(channels[:-1], channels[1:], ksize):
        params += [rn(co, ci, k, k) / (ci * k * k) ** 0.5, 0.3 * rn(co), 0.5 + torch.rand(co, generator=gen, dtype=torch.float64), 0.5 * rn(co)]
        running += [0.5 * rn(co), 0.5 + torch.rand(co, generator=gen, dtype=torch.float64)]
    return rn(N, channels[0], H, W), rn(N, channels[-1], H, W), params, running


def module_chain(channels, ksize, params, running):
    layers = []
    for i, (ci, co, k) in enumerate(zip(channels[:-1], channels[1:], ksize)):
        c = torch.nn.Conv2d(ci, co, k, padding=k // 2).double()
        b = torch.nn.BatchNorm2d(co, eps=R.EPS, momentum=R.MOMENTUM).double()
        with torch.no_grad():
            c.weight.copy_(params[4 * i]); c.bias.copy_(params[4 * i + 1]); b.weight.copy_(params[4 * i + 2]); b.bias.copy_(params[4 * i + 3])
            b.running_mean.copy_(running[2 * i]); b.running_var.copy_(running[2 * i + 1])
        layers += [c, b, torch.nn.ReLU()]
    return torch.nn.Sequential(*layers)


CASES = [(c, k, s) for c, k in CHAINS for s in SHAPES]


@pytest.mark.parametrize("channels,ksize,shape", CASES)
@pytest.mark.parametrize("training", [True, False])
def test_free_forward_is_the_module_chain_and_teacher_forcing_agrees(channels, ksize, shape, training):
    x, _, params, running = make(channels, ksize, shape, 1)
    m = module_chain(channels, ksize, params, running).train(training)
    y, state, new_running = R.forward_free(x, params, running, training)
    assert R.relmax(y, m(x)) < 1e-12
    bns = [l for l in m if isinstance(l, torch.nn.BatchNorm2d)]
    for i, b in enumerate(bns):          # the running-statistics update (eval mode: untouched)
        assert R.relmax(new_running[2 * i], b.running_mean) < 1e-12 and R.relmax(new_running[2 * i + 1], b.running_var) < 1e-12
        if not training:
            assert torch.equal(new_running[2 * i], running[2 * i]) and torch.equal(new_running[2 * i + 1], running[2 * i + 1])
    # teacher-forced at the chain's own state = the free-running chain; the output is the last state's ReLU
    for z, (zs, _, _) in zip(R.forward_teacher(x, params, state), state):
        assert R.relmax(z, zs) < 1e-12
    assert torch.equal(R.output(state), y)
    # the vectors of a block from its stored z
    for i, (z, sc, sh) in enumerate(state):
        v = R.bn_vectors(z, params[4 * i + 2], params[4 * i + 3], running[2 * i], running[2 * i + 1], training)
        assert torch.equal(v["sc"], sc) and torch.equal(v["sh"], sh)
        assert R.relmax(v["asc"] * v["mean"], -v["ash"]) < 1e-12 and R.relmax(v["asc"], 1 / torch.sqrt(v["var"] + R.EPS)) < 1e-12


@pytest.mark.parametrize("channels,ksize,shape", CASES)
@pytest.mark.parametrize("training", [True, False])
def test_straight_through_backward_at_own_state_is_autograd(channels, ksize, shape, training):
    x, gy, params, running = make(channels, ksize, shape, 2)
    _, state, _ = R.forward_free(x, params, running, training)
    gx, grads, gz = R.backward_straight_through(x, gy, params, running, state, training)
    m = module_chain(channels, ksize, params, running).train(training)
    xl = x.clone().requires_grad_(True)
    (m(xl) * gy).sum().backward()
    assert R.relmax(gx, xl.grad) < 1e-12
    ref = [p.grad for l in m if not isinstance(l, torch.nn.ReLU) for p in (l.weight, l.bias)]
    assert len(ref) == len(grads)
    for i, (g, r) in enumerate(zip(grads, ref)):
        if training and i % 4 == 1:       # a conv bias in front of a train-mode BatchNorm: both are rounding noise around zero
            assert float(g.abs().max()) < 1e-12 * float(grads[i - 1].norm()) and float(r.abs().max()) < 1e-12 * float(grads[i - 1].norm())
        else:
            assert R.relmax(g, r) < 1e-12, i
    assert len(gz) == len(ksize) and all(g.shape == s[0].shape for g, s in zip(gz, state))


def test_straight_through_uses_the_states_values_and_masks():
    """A state that is NOT the chain's own: the mask and the value come from the state, the derivative from the convolution."""
    channels, ksize = (16, 16, 16), (3, 3)
    x, gy, params, running = make(channels, ksize, (2, 4, 8), 3)
    _, state, _ = R.forward_free(x, params, running, False)
    flipped = [(-z, sc, sh) for z, sc, sh in state]
    gx, grads, gz = R.backward_straight_through(x, gy, params, running, flipped, False)
    # by hand, eval mode: g_z1 = gy * mask1 * s1; g_a0 = conv^T(g_z1); g_z0 = g_a0 * mask0 * s0
    s = [params[4 * i + 2] / torch.sqrt(running[2 * i + 1] + R.EPS) for i in range(2)]
    mask = [((-z) * R._c(sc) + R._c(sh) > 0).double() for z, sc, sh in state]
    gz1 = gy * mask[1] * R._c(s[1])
    ga0 = torch.nn.functional.conv_transpose2d(gz1, params[4], padding=1)
    gz0 = ga0 * mask[0] * R._c(s[0])
    assert R.relmax(gz[1], gz1) < 1e-12 and R.relmax(gz[0], gz0) < 1e-12
    assert R.relmax(gx, torch.nn.functional.conv_transpose2d(gz0, params[0], padding=1)) < 1e-12
    assert R.relmax(grads[5], gz1.sum((0, 2, 3))) < 1e-12
    # d/d gamma_1 reads the STATE's z: sum gy * mask * xhat(-z)
    xhat = (-state[1][0] - R._c(running[2])) / torch.sqrt(R._c(running[3]) + R.EPS)
    assert R.relmax(grads[6], (gy * mask[1] * xhat).sum((0, 2, 3))) < 1e-12


@pytest.mark.parametrize("channels,ksize,shape", CASES)
def test_folded_form_is_eval_mode(channels, ksize, shape):
    x, _, params, running = make(channels, ksize, shape, 4)
    y, _, _ = R.forward_free(x, params, running, False)
    assert R.relmax(R.folded(x, params, running), y) < 1e-12


def test_fp32_baseline_is_close_to_fp64():
    channels, ksize = (16, 48, 64, 16), (3, 3, 3)
    x, gy, params, running = make(channels, ksize, (3, 6, 20), 5)
    x, gy, params, running = x.float(), gy.float(), R.cast(params, torch.float32), R.cast(running, torch.float32)
    _, state, _ = R.forward_free(x, params, running, True)
    z64, z32 = R.forward_teacher(x, params, state), R.forward_teacher(x, params, state, torch.float32)
    assert all(z.dtype == torch.float32 for z in z32)
    assert all(0 < R.relmax(a, b) < 1e-5 for a, b in zip(z32, z64))
    assert 0 < R.relmax(R.folded(x, params, running, dtype=torch.float32), R.folded(x, params, running)) < 1e-5
