"""Gradient-norm clipping on the device (``lf_grad_sumsq`` / ``lf_grad_norm_finish`` / ``lf_grad_scale_inplace`` and the
``lf_*_step_clipped`` launches) in the layout of tests/test_optim_gpu.py: gradients as views of one flat buffer at every offset
residue mod 4, tails of 1 / 3 / 255 / 4095 / 4097 / 12289 elements, a parameter without a gradient, sentinel guards around
everything.  The norm is held to ``grad_scale * sqrt(sum g**2)`` evaluated in fp64 within 2 * 2**-24 relative (tests/clip_ref.py:
an fp64 accumulation plus the one rounding to fp32), the clipped steps to the unchanged fp64
yardstick of tests/optim_ref.py with ``grad_scale_eff = grad_scale * coef``, and the two forms of the clip to each other bit for
bit.

Largest observed on an MI355X (for the record; the assertions are the bounds): |total_norm - fp64| at 0.34 of its gate; clipped
steps |kernel - fp64| / bound p 0.999, m 0.31, v 0.12 over the 72 one-step cases and the ten-step runs (the p bound opens with the
final rounding of p - update, which a correctly rounded subtraction reaches, as in tests/test_optim_gpu.py).
"""
import copy
import importlib
from argparse import Namespace

import numpy as np
import pytest
import torch

import clip_ref as C
import optim_ref as R
from test_optim_gpu import SENTINEL, STATE_NAMES, Layout, _compare, _groups
from test_main_loop_gpu import _tree_on_path

pytestmark = pytest.mark.gpu

MAX_NORMS = (1e-3, 1.0, 100.0)


@pytest.fixture()
def bp_tree_on_path():
    yield from _tree_on_path("bp")                                         # the mirrored BP tree first on sys.path


@pytest.fixture(scope="module")
def inputs():
    data = R.make_inputs(0)
    for t in data:
        for a in t.values():
            a.setflags(write=False)
    return data


def _make(kind, groups, grad_scale, max_grad_norm=0.0):
    from lanedetection_end2end_amd.optim import FusedAdam, FusedRMSprop, FusedSGD
    return {"adam": FusedAdam, "sgd": FusedSGD, "rmsprop": FusedRMSprop}[kind](groups, grad_scale=grad_scale, max_grad_norm=max_grad_norm)


def _one_group(lay, wd=0.0):
    return [dict(params=lay.module_order, lr=R.LR, weight_decay=wd)]


def _read(opt):
    """(total_norm, coef) of the last clipped step as np.float32."""
    assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.dtype == torch.float32 and opt.last_grad_norm.is_cuda
    return np.float32(opt.last_grad_norm.item()), np.float32(opt.last_clip_coef.item())


def _bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def _check_norm(total, grads, grad_scale, what=""):
    want = C.norm_f64(grads, grad_scale)
    err = abs(float(total) - want)
    print("%s total_norm %.9g, fp64 %.12g: %.3f of the bound" % (what, float(total), want, err / (C.NORM_TOL * want) if want else 0.0))
    assert np.isfinite(total) and err <= C.NORM_TOL * want, (float(total), want)
    return want


def _same_state(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        for n in "pmv":
            assert np.array_equal(_bits(x[n]), _bits(y[n])), "tensor %d, %s differs" % (i, n)


@pytest.mark.parametrize("two_groups", [False, True], ids=["one-group", "two-groups"])
@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_norm_matches_fp64(inputs, grad_scale, two_groups):
    """The global norm over every group, twice on the cached table and once on a rebuilt one: within the bound, and the same bits."""
    lay = Layout(inputs)
    opt = _make("sgd", _groups(lay) if two_groups else _one_group(lay), grad_scale, 1.0)
    lay.install()
    flat_before = lay.flat.clone()
    grads = [t["g"] for t in inputs]
    opt.step()
    first = _read(opt)
    want = _check_norm(first[0], grads, grad_scale, "gs %g:" % grad_scale)
    assert abs(want - 2730.2 * grad_scale) < 0.05 * grad_scale
    assert first[1].tobytes() == C.coef(first[0], 1.0).tobytes() and first[1] < 1
    tables = dict(opt._tables)
    opt.step()
    assert all(opt._tables[g] is tables[g] for g in tables), "the device table was rebuilt: this is not the cached path"
    second = _read(opt)
    opt._tables = {}
    opt.step()
    assert all(opt._tables[g] is not tables[g] for g in tables)
    third = _read(opt)
    for other in (second, third):
        assert other[0].tobytes() == first[0].tobytes() and other[1].tobytes() == first[1].tobytes()
    lay.assert_untouched(flat_before)


def test_squares_do_not_overflow(inputs):
    """1e30 and -3e30: their squares are Inf in fp32, the norm 3.1623e30 is not."""
    data = [dict(t) for t in inputs]
    for i, at, val in ((0, 1021, 1e30), (7, 8190, -3e30)):                # a vector-form full chunk, a tail
        g = data[i]["g"].copy()
        g[at] = val
        data[i]["g"] = g
    lay = Layout(data)
    opt = _make("sgd", _one_group(lay), 1.0, 1.0)
    lay.install()
    opt.step()
    total, coef = _read(opt)
    want = _check_norm(total, [t["g"] for t in data], 1.0)
    assert abs(want - 3.1623e30) < 1e26 and coef.tobytes() == C.coef(total, 1.0).tobytes() and 0 < coef < 1e-29


@pytest.mark.parametrize("max_norm", MAX_NORMS)
@pytest.mark.parametrize("kind,wd,grad_scale,k", R.VALUE_CASES,
                         ids=["%s-wd%g-gs%g%s" % (c[0], c[1], c[2], "" if c[3] is None else "-step%d" % c[3]) for c in R.VALUE_CASES])
def test_clipped_step_matches_fp64(kind, wd, grad_scale, k, max_norm, inputs):
    """ONE clipped step from a seeded fp32 state: with the coefficient the device computed, p and both moments sit inside the
    UNCHANGED bound of tests/optim_ref.py around the fp64 step taken with grad_scale * coef; nothing else is written."""
    lay = Layout(inputs)
    opt = _make(kind, _one_group(lay, wd), grad_scale, max_norm)
    lay.seed_state(opt, kind, 0 if k is None else k - 1)
    lay.install()
    before, flat_before = lay.snapshot(opt, kind), lay.flat.clone()
    opt.step()
    after = lay.snapshot(opt, kind)
    total, coef = _read(opt)
    _check_norm(total, [t["g"] for t in inputs], grad_scale)
    assert coef.tobytes() == C.coef(total, max_norm).tobytes() and 0 < coef < 1
    n = len(lay.params)
    worst = _compare(kind, before, after, [R.hyper(kind, R.LR, wd)] * n, grad_scale * float(coef), [k] * n)
    print("%s wd=%g grad_scale=%g step=%s max_norm=%g: kernel / bound  p %.3f  m %.2f  v %.2f" % (
        kind, wd, grad_scale, k, max_norm, worst["p"], worst["m"], worst["v"]))
    lay.assert_untouched(flat_before)
    assert all(opt.state[p]["step"] == (1 if k is None else k) for p in lay.params)


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("kind", R.KINDS)
def test_drop_in_then_step_equals_fused_step(kind, wd, grad_scale, inputs):
    """``clip_grad_norm_`` followed by an unclipped step, and the clipped step from the same state: the same bits in p and in the
    state.  After the drop-in call every gradient is fl32(fl32(g * grad_scale) * coef), bit for bit, and the gaps and the tail of
    the flat buffer still hold the sentinel."""
    from lanedetection_end2end_amd import optim
    a, b = Layout(inputs), Layout(inputs)
    plain = _make(kind, _one_group(a, wd), 1.0)
    fused = _make(kind, _one_group(b, wd), grad_scale, 1.0)
    for lay, opt in ((a, plain), (b, fused)):
        lay.seed_state(opt, kind, 2)
        lay.install()
    flat_before = a.flat.clone()
    total = optim.clip_grad_norm_(a.module_order, 1.0, grad_scale=grad_scale)
    assert total.is_cuda and total.dim() == 0 and total.dtype == torch.float32
    total = np.float32(total.item())
    _check_norm(total, [t["g"] for t in inputs], grad_scale)
    coef = C.coef(total, 1.0)
    for t, g in zip(inputs, a.grads):
        assert np.array_equal(_bits(g.cpu().numpy().ravel()), _bits(C.effective(t["g"], grad_scale, coef)))
    assert bool((a.flat[a.gap] == SENTINEL).all()) and not torch.equal(a.flat, flat_before)
    flat_clipped = a.flat.clone()
    plain.step()
    a.assert_untouched(flat_clipped)
    flat_b = b.flat.clone()
    fused.step()
    b.assert_untouched(flat_b)
    got = _read(fused)
    assert got[0].tobytes() == total.tobytes() and got[1].tobytes() == coef.tobytes()
    _same_state(a.snapshot(plain, kind), b.snapshot(fused, kind))


@pytest.mark.parametrize("kind", R.KINDS)
def test_below_the_threshold_nothing_changes(kind, inputs):
    """max_norm above the norm (2730.2): coef is exactly 1 and the clipped step leaves the bits of an optimizer built without
    clipping."""
    a, b = Layout(inputs), Layout(inputs)
    plain, fused = _make(kind, _groups(a), 0.125), _make(kind, _groups(b), 0.125, 1e4)
    for lay, opt in ((a, plain), (b, fused)):
        lay.seed_state(opt, kind, 2)
        lay.install()
    plain.step()
    fused.step()
    total, coef = _read(fused)
    assert coef == 1.0 and abs(float(total) - 2730.2 * 0.125) < 0.01
    assert plain.last_grad_norm is None
    _same_state(a.snapshot(plain, kind), b.snapshot(fused, kind))


def test_non_finite_gradients_are_torchs(inputs):
    """torch's clip_grad_norm_(error_if_nonfinite=False), no skip: an Inf gradient gives norm Inf and coef 0 -- every finite
    gradient then counts as zero and the Inf element becomes NaN; a NaN gradient gives a NaN coefficient (not 1); all-zero gradients
    give norm 0, coef 1 and no NaN."""
    kind, at = "adam", (2, 5)                                              # tensor 2 (4097 elements, scalar form), element 5
    data = [dict(t) for t in inputs]
    g = data[at[0]]["g"].copy()
    g[at[1]] = np.inf
    data[at[0]]["g"] = g
    zeros = [dict(t, g=np.zeros_like(t["g"])) for t in inputs]
    a, b = Layout(data), Layout(zeros)
    clipped, plain = _make(kind, _one_group(a, 1e-2), 1.0, 1.0), _make(kind, _one_group(b, 1e-2), 1.0)
    for lay, opt in ((a, clipped), (b, plain)):
        lay.seed_state(opt, kind, 2)
        lay.install()
    flat_before = a.flat.clone()
    clipped.step()
    plain.step()
    total, coef = _read(clipped)
    assert np.isinf(total) and total > 0 and coef == 0
    got, zero = a.snapshot(clipped, kind), b.snapshot(plain, kind)
    for i, (x, y) in enumerate(zip(got, zero)):
        keep = np.ones(len(x["p"]), bool)
        if i == at[0]:
            keep[at[1]] = False
            assert all(np.isnan(x[n][at[1]]) for n in "pmv")
        for n in "pmv":
            assert np.array_equal(x[n][keep], y[n][keep]), (i, n)
    a.assert_untouched(flat_before)

    g[at[1]] = np.nan
    lay = Layout(data)
    opt = _make(kind, _one_group(lay), 1.0, 1.0)
    lay.install()
    opt.step()
    total, coef = _read(opt)
    assert np.isnan(total) and np.isnan(coef)
    assert all(np.isnan(t[n]).all() for t in lay.snapshot(opt, kind) for n in "pmv")

    lay = Layout(zeros)
    opt = _make(kind, _one_group(lay), 1.0, 1.0)
    lay.install()
    opt.step()
    total, coef = _read(opt)
    assert total == 0 and coef == 1
    assert all(np.isfinite(t[n]).all() for t in lay.snapshot(opt, kind) for n in "pmv")


@pytest.mark.parametrize("kind", R.KINDS)
def test_ten_clipped_steps_cached_tables_late_starter_and_reload(kind, inputs):
    """Ten clipped steps with fresh gradient values written in place, two param groups; one tensor gets its first gradient at
    step 3 (its values sit in the flat buffer before that and must not enter the norm), and the state is reloaded through
    ``load_state_dict`` after step 6.  After EVERY step: the norm of the tensors that took part, the coefficient, and p / m / v
    inside the fp64 bound with the bias correction of each tensor's own count."""
    lay = Layout(inputs)
    late, gs = 7, 0.125
    opt = _make(kind, _groups(lay), gs, 1.0)
    lay.install(only=set(range(len(lay.params))) - {late})
    counts = [0] * len(lay.params)
    worst = dict(p=0.0, m=0.0, v=0.0)
    for step in range(1, 11):
        if step == 3:
            lay.install(only={late})
        if step == 7:
            opt.load_state_dict(copy.deepcopy(opt.state_dict()))
            assert not opt._tables
        fresh = [t["g"] for t in R.make_inputs(200 + step)]
        lay.set_grads(fresh)
        before, flat_before = lay.snapshot(opt, kind), lay.flat.clone()
        tables = dict(opt._tables)
        opt.step()
        if step not in (1, 3, 7):
            assert all(opt._tables[g] is tables[g] for g in tables), "step %d rebuilt a table" % step
        after = lay.snapshot(opt, kind)
        total, coef = _read(opt)
        _check_norm(total, [g for g, p in zip(fresh, lay.params) if p.grad is not None], gs, "step %d:" % step)
        assert coef.tobytes() == C.coef(total, 1.0).tobytes()
        hps = []
        for i, p in enumerate(lay.params):
            group = next(g for g in opt.param_groups if any(q is p for q in g["params"]))
            has = p.grad is not None
            counts[i] += has
            hps.append(R.hyper(kind, group["lr"], group["weight_decay"]) if has else None)
        w = _compare(kind, before, after, hps, gs * float(coef), counts)
        worst = {n: max(worst[n], w[n]) for n in w}
        lay.assert_untouched(flat_before)
        for p, c in zip(lay.params, counts):
            assert (int(opt.state[p]["step"]) == c) if c else (not opt.state.get(p))
    assert counts == [8 if i == late else 10 for i in range(len(lay.params))]
    print("%s ten clipped steps: kernel / bound  p %.3f  m %.2f  v %.2f" % (kind, worst["p"], worst["m"], worst["v"]))


def _bp_loop(form, steps=3):
    """The train-step statements of BP/main.py:232-340 (as tests/test_main_loop_gpu.py::test_bp_main_loop_body has them) at its
    small shape with ``clip_grad_norm = 1``: ``form`` "fused" builds the optimizer with ``define_optim(..., clip_grad_norm=1)``,
    "drop-in" calls ``clip_grad_norm`` where main.py:334-335 does.  -> parameters after the last step, (norm, fp64 norm) per step."""
    from lanedetection_end2end_amd import optim
    from oracle import inputs as synth
    Net = importlib.import_module("Networks.LSQ_layer").Net
    define_loss_crit = importlib.import_module("Loss_crit").define_loss_crit
    N, R_, nclasses = 2, 64, 4
    args = Namespace(batch_size=N, nclasses=nclasses, resize=R_, end_to_end=True, mod="erfnet", layers=18, channels_in=3,
                     pretrained=True, pool=True, activation_layer="square", no_cuda=False, order=2, reg_ls=0.0,
                     use_cholesky=False, mask_percentage=0.2, clas=False, no_mapping=False, loss_policy="backproject",
                     weight_funct="none", weight_seg=30, optimizer="adam", learning_rate=1e-4, weight_decay=0.0,
                     clip_grad_norm=1, weight_fit=1.0, weight_class=1.0)
    torch.manual_seed(5)
    model = Net(args).cuda()
    if form == "fused":
        optimizer = optim.define_optim(args.optimizer, model.parameters(), args.learning_rate, args.weight_decay,
                                       clip_grad_norm=args.clip_grad_norm)
    else:
        optimizer = optim.define_optim(args.optimizer, model.parameters(), args.learning_rate, args.weight_decay)
    criterion, criterion_seg = define_loss_crit(args)
    model.train()
    schedule = [(True, False), (False, False), (False, True)][:steps]      # skip epoch, segmentation mode, end to end
    norms = []
    for i, (skip, end_to_end) in enumerate(schedule):
        args.end_to_end = end_to_end
        lanes, valid = synth.bp_targets(N, 4, R_, seed=700 + i)
        input = torch.from_numpy(synth.images(N, R_, 2 * R_, seed=300 + i)).cuda()
        gt = torch.from_numpy(synth.seg_targets(N, R_, 2 * R_, nclasses + 1, seed=500 + i)).cuda()
        lanes, valid_points, gt_line = torch.from_numpy(lanes).cuda(), torch.from_numpy(valid).cuda(), torch.zeros(N, 4)
        if skip:                                                           # main.py:254-262
            loss = criterion_seg(model(input, gt_line, args.end_to_end, early_return=True), gt)
        else:
            beta0, beta1, beta2, beta3, _, output_net, _, _, _ = model(input, gt_line, args.end_to_end, gt=gt)
            if args.end_to_end:                                            # main.py:296-305
                loss_left = criterion(beta0, lanes[:, 0], valid_points[:, 0])[0] + criterion(beta2, lanes[:, 2], valid_points[:, 2])[0]
                loss_right = criterion(beta1, lanes[:, 1], valid_points[:, 1])[0] + criterion(beta3, lanes[:, 3], valid_points[:, 3])[0]
                loss = (loss_left + loss_right) / args.nclasses
            else:                                                          # main.py:306-307
                loss = criterion_seg(output_net, gt)
        optimizer.zero_grad()                                              # main.py:338-340, the clip of :334-335 in between
        loss.backward()
        want = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None)))
        if form == "drop-in" and args.clip_grad_norm != 0:
            total = optim.clip_grad_norm(model.parameters(), args.clip_grad_norm)
        optimizer.step()
        if form == "fused":
            total = optimizer.last_grad_norm
        norms.append((float(total), want))
    criterion_seg.flush()
    return [p.detach().clone() for p in model.parameters()], norms


def test_bp_loop_with_clipping(bp_tree_on_path):
    """Three steps of the BP loop with ``--clip_grad_norm 1``, once with the clip inside ``optimizer.step()`` and once with the
    drop-in call in main.py's place: the same parameters bit for bit, and every step's norm is the fp64 norm of that step's
    gradients."""
    fused, norms_f = _bp_loop("fused")
    plain, norms_d = _bp_loop("drop-in")
    for (got, want), (got_d, want_d) in zip(norms_f, norms_d):
        print("norm %.9g (fused) %.9g (drop-in), fp64 %.12g" % (got, got_d, want))
        assert np.isfinite(want) and want > 0 and want == want_d
        assert abs(got - want) <= C.NORM_TOL * want and got_d == got
    assert len(fused) == len(plain) > 200
    for i, (x, y) in enumerate(zip(fused, plain)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "parameter %d differs between the two forms" % i
