"""The --clas heads and only_encode in the bf16 precision mode (Net.precision = "bf16"): the recipe of
Backprojection_Loss/train.sh (--nclasses 4 --order 3 --clas 1) trains end to end with the heads on the bf16 encoder output.

The reference has no reduced-precision mode, so the gates are bf16-level: every comparison is against fp64 on the same
bf16-rounded operands (inputs, upstream gradients, convolution weights), and a train-mode BatchNorm backward -- whose
output is a difference of nearly equal sums -- gets the looser gate, as test_bf16_blocks_at_config3_shapes reasons.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import clas_oracle, erfnet_oracle, inputs
from oracle.gen_golden_clas import clas_inputs

pytestmark = pytest.mark.gpu

B7, B5 = 2.0 ** -7, 2.0 ** -5


def _l2(a, b):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _round_weights(P):
    """Convolution / linear weights rounded to bf16 (what the bf16 matrix cores multiply); BatchNorm vectors and biases stay."""
    return type(P)((k, _bf16(v) if (k.endswith(".weight") and v.dim() >= 2) else v.clone()) for k, v in P.items())


def _bp_args(N, R, K, clas, precision, order=3):
    from argparse import Namespace
    return Namespace(batch_size=N, nclasses=K, resize=R, end_to_end=True, mod="erfnet", layers=18, channels_in=3,
                     pretrained=False, pool=True, activation_layer="square", no_cuda=False, order=order, reg_ls=0.0,
                     use_cholesky=False, mask_percentage=0.2, clas=clas, no_mapping=False, loss_policy="backproject",
                     weight_seg=30, weight_funct="none", precision=precision, weight_fit=1.0, weight_class=1.0)


def _recipe_model(N, R, K, precision, seed=5):
    from lanedetection_end2end_amd.bp.Networks.LSQ_layer import Net
    args = _bp_args(N, R, K, True, precision)
    model = Net(args)
    model.net.load_state_dict(erfnet_oracle.make_params(seed=seed, out_channels=K))
    model.line_classification.load_state_dict(clas_oracle.make_clas_params("line", seed=11))
    model.horizon_estimation.load_state_dict(clas_oracle.make_clas_params("horizon", seed=12))
    model = model.cuda()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0
    return model.train(), args


def _recipe_data(N, R, K, seed=71):
    x = torch.from_numpy(inputs.images(N, R, 2 * R, seed=seed)).cuda()
    lanes, valid = inputs.bp_targets(N, K, R, seed=seed + 1)
    rng = np.random.default_rng(seed)
    gt_line = torch.from_numpy((rng.uniform(0, 1, (N, 4)) > 0.5).astype(np.float32)).cuda()
    gt_hor = torch.from_numpy((rng.uniform(0, 1, (N, R)) > 0.5).astype(np.float32)).cuda()
    lt = [torch.from_numpy(lanes[:, k]).cuda() for k in range(K)]
    vt = [torch.from_numpy(valid[:, k]).cuda() for k in range(K)]
    return x, lt, vt, gt_line, gt_hor


def _recipe_loss(model, args, crit, data, heads=True):
    """BP/main.py:295-326: backprojection loss over the lanes / nclasses, + line and horizon BCE (weight_fit = weight_class = 1)."""
    x, lt, vt, gt_line, gt_hor = data
    K = args.nclasses
    out = model(x, torch.zeros(x.shape[0], K), True)
    betas, line, horizon, output_seg = out[:4], out[6], out[7], out[8]
    loss = sum(crit(betas[k], lt[k], vt[k])[0] for k in range(K)) / K
    parts = [loss]
    if heads:
        bce = torch.nn.BCEWithLogitsLoss()
        l_line, l_hor = bce(line, gt_line).double(), bce(horizon, gt_hor).double()
        parts += [l_line, l_hor]
        loss = loss * args.weight_fit + (l_line + l_hor) * args.weight_class
    return loss, parts, (line, horizon, output_seg)


def test_train_sh_recipe_step_in_bf16():
    """One training step of the train.sh recipe (BP Net, clas=1, nclasses=4, order=3) at 256 x 512, batch 8, in bf16: losses
    and gradients finite, the same parameters receive gradients as in fp32, FusedAdam steps, and the heads' gradient reaches the
    encoder (its gradients differ from those of the fit loss alone)."""
    from lanedetection_end2end_amd.bp.Loss_crit import backprojection_loss
    from lanedetection_end2end_amd.optim import FusedAdam
    N, R, K = 8, 256, 4
    data = _recipe_data(N, R, K)
    with_grad = {}
    for precision in ("fp32", "bf16"):
        model, args = _recipe_model(N, R, K, precision)
        crit = backprojection_loss(args)
        loss, parts, (line, horizon, seg) = _recipe_loss(model, args, crit, data)
        assert line.dtype == torch.float32 and horizon.dtype == torch.float32 and line.shape == (N, 4) and horizon.shape == (N, R)
        assert seg.dtype == (torch.bfloat16 if precision == "bf16" else torch.float32) and seg.shape == (N, 128, R // 8, R // 4)
        model.zero_grad(set_to_none=True)
        loss.backward()
        assert all(torch.isfinite(p).all() for p in parts), (precision, [float(p) for p in parts])
        with_grad[precision] = {k for k, p in model.named_parameters() if p.grad is not None}
        for k, p in model.named_parameters():
            if p.grad is not None:
                assert p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), (precision, k)
        assert float(model.line_classification.conv2.weight.grad.abs().max()) > 0
        assert float(model.horizon_estimation.fully_connected_horizon.weight.grad.abs().max()) > 0
        if precision == "bf16":
            k_enc = "net.encoder.layers.14.conv1x3_2.weight"
            g_all = dict(model.named_parameters())[k_enc].grad.clone()
            before = [p.detach().clone() for p in model.parameters()]
            nonzero = sum(int(p.grad is not None and bool(p.grad.abs().max() > 0)) for p in model.parameters())
            opt = FusedAdam([p for p in model.parameters()], lr=1e-4)
            opt.step()
            moved = sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, model.parameters()))
            assert moved == nonzero, (moved, nonzero)          # (Adam leaves a parameter whose first gradient is exactly 0)
            assert all(torch.isfinite(p).all() for p in model.parameters())
            # the same forward state without the two head losses, twice: the encoder gradient changes by far more than two
            # evaluations of one loss differ -- the injected term is used (the fit loss is ~2e4 here, the head losses ~1)
            g_fit = []
            for _ in range(2):
                model2, _ = _recipe_model(N, R, K, precision)
                loss2, _, _ = _recipe_loss(model2, args, crit, data, heads=False)
                loss2.backward()
                g_fit.append(dict(model2.named_parameters())[k_enc].grad)
            d, noise = _l2(g_all, g_fit[0]), _l2(g_fit[1], g_fit[0])
            print("bf16 recipe step: losses %s; encoder gradient with / without the heads differ by %.2e (relative L2), "
                  "two runs without them by %.2e" % (["%.4f" % float(p) for p in parts], d, noise))
            assert d > 1e-4 and d > 10 * noise
    assert with_grad["bf16"] == with_grad["fp32"], sorted(with_grad["bf16"] ^ with_grad["fp32"])


@pytest.mark.parametrize("tree", ["bp", "bev"])
def test_trunk_bf16_against_fp64(tree):
    """conv1..conv4 (+BN+ReLU) in the chain's bf16 mode against the fp64 oracle trunk on the same bf16-rounded input, upstream
    gradient and convolution weights.  Forward: relative L2 < 2^-7 (train and eval).  Backward in eval mode (affine BatchNorm):
    d/d input and every parameter gradient < 2^-7.  Backward in train mode: the data / weight gradients above the last BatchNorm are
    differences of nearly equal sums (the BatchNorm backward's mean subtraction), held to 2^-5; the last BatchNorm's own
    gamma / beta gradients to 2^-7."""
    if tree == "bev":
        from lanedetection_end2end_amd.bev.Networks.LSQ_layer import Classification
    else:
        from lanedetection_end2end_amd.bp.Networks.LSQ_layer import Classification
    x, _ = clas_inputs("horizon", tree)
    x = _bf16(torch.from_numpy(x))
    P32 = _round_weights(clas_oracle.make_clas_params("line", seed=7, tree=tree))
    m = Classification("line", size=(32, 64), channels_in=128, resize=256)
    m.load_state_dict(P32)
    m = m.cuda()
    g = _bf16(torch.from_numpy(np.random.default_rng(3).standard_normal((x.shape[0], 32, 64, 64)).astype(np.float32)))
    trunk_keys = [k for k in P32 if k.startswith("conv") and "running" not in k and "num_batches" not in k]
    N, H, W = x.shape[0], 32, 64
    for training in (True, False):
        m.train(training)
        for p in m.parameters():
            p.grad = None
        # the module's state as this forward sees it (the eval pass uses the running statistics the train pass updated)
        Pd = clas_oracle.cast_params({k: v.detach().cpu() for k, v in m.state_dict().items()}, torch.float64)
        xt = x.cuda().permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).permute(0, 3, 1, 2).requires_grad_(True)
        y = m.trunk(xt)
        assert y.dtype == torch.bfloat16 and y.shape == (x.shape[0], 32, 64, 64)
        state = _chain_state(y.grad_fn.ws, N, H, W, m._channels, m._plans[(N, H, W)])
        (y.float() * g.cuda()).sum().backward()
        assert xt.grad.dtype == torch.bfloat16
        with torch.no_grad():
            yo = clas_oracle.classification_trunk(x.double(), Pd, training)
        e_y = _l2(y.permute(0, 3, 1, 2), yo)
        for k in trunk_keys:
            Pd[k].requires_grad_(True)
        xo = x.double().requires_grad_(True)
        yst = _trunk_straight_through(xo, Pd, training, state)
        (yst.permute(0, 2, 3, 1) * g.double()).sum().backward()
        e_x = _l2(xt.grad, xo.grad)
        errs = {k: _l2(dict(m.named_parameters())[k].grad, Pd[k].grad) for k in trunk_keys
                if not (training and k.endswith(".bias") and "_bn" not in k)}       # (a bias before a train-mode BatchNorm: zero)
        worst = max(errs, key=errs.get)
        print("%s trunk, %s: forward %.2e, d/d input %.2e, worst parameter gradient %.2e (%s)" % (
            tree, "train" if training else "eval", e_y, e_x, errs[worst], worst))
        assert e_y < B7
        if training:
            assert e_x < B5 and all(e < B5 for e in errs.values()), errs
            assert errs["conv4_bn.weight"] < B7 and errs["conv4_bn.bias"] < B7
        else:
            assert e_x < B7 and all(e < B7 for e in errs.values()), errs
        if training:
            sd = m.state_dict()
            assert int(sd["conv4_bn.num_batches_tracked"]) == 1


def _chain_state(ws, N, H, W, channels, plan):
    """The conv chain's saved forward state in its workspace, found with lf_debug_convchain_offset (csrc/lf_debug.h: float offsets
    of block i's pre-BN tensor z and of its folded BatchNorm scale and shift): per block (z as stored -- bf16 in mode 2 --, scale,
    shift) in fp64."""
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    npix, out = N * H * W, []
    for i, co in enumerate(channels[1:]):
        oz, osc, osh = (lib.lf_debug_convchain_offset(plan.handle, i, which) for which in (0, 1, 2))
        assert min(oz, osc, osh) >= 0
        z = ws.view(torch.bfloat16)[2 * oz: 2 * oz + npix * co].view(N, H, W, co).permute(0, 3, 1, 2).double().cpu()
        sc = ws.view(torch.float32)[osc: osc + co].double().cpu()
        sh = ws.view(torch.float32)[osh: osh + co].double().cpu()
        out.append((z, sc, sh))
    return out


def _trunk_straight_through(x, P, training, state):
    """The fp64 trunk evaluated straight-through at the engine's forward state: every pre-BN tensor takes the engine's VALUE (its
    derivative stays the fp64 convolution's) and every ReLU the engine's mask, sign(z * scale + shift) of the stored z with the
    folded fp32 vectors the engine decided it with -- the gradient differences left are backward arithmetic."""
    import torch.nn.functional as F
    for name, (ze, sc, sh) in zip(("conv1", "conv2", "conv3", "conv4"), state):
        w = P[name + ".weight"]
        z = F.conv2d(x, w, P[name + ".bias"], padding=(w.shape[2] - 1) // 2)
        z = z + (ze - z).detach()
        if training:
            mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        else:
            mean, var = P[name + "_bn.running_mean"], P[name + "_bn.running_var"]
        a = (z - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + clas_oracle.BN_EPS)
        a = a * P[name + "_bn.weight"][None, :, None, None] + P[name + "_bn.bias"][None, :, None, None]
        x = a * ((ze * sc[None, :, None, None] + sh[None, :, None, None]) > 0).double()
    return x


# relative L2 to the fp64 goldens (which use the unrounded weights), measured on MI355X: line 7.0e-3 / 4.8e-3 (BP, train / eval),
# 7.8e-3 / 6.1e-3 (BEV), horizon 2.8e-3 / 2.4e-3 -- the bound is ~4x the worst
GOLDEN_BOUND = 3e-2


@pytest.mark.parametrize("tree,class_type", [("bp", "line"), ("bp", "horizon"), ("bev", "line"), ("bev", "horizon")])
def test_heads_bf16_against_goldens(tree, class_type):
    if tree == "bev":
        from lanedetection_end2end_amd.bev.Networks.LSQ_layer import Classification
        gold = np.load(os.path.join(GOLDEN, "clas_bev.npz" if class_type == "line" else "clas.npz"), allow_pickle=False)
    else:
        from lanedetection_end2end_amd.bp.Networks.LSQ_layer import Classification
        gold = np.load(os.path.join(GOLDEN, "clas.npz"), allow_pickle=False)
    x, _ = clas_inputs(class_type, tree)
    P32 = clas_oracle.make_clas_params(class_type, seed=7, tree=tree if class_type == "line" else "bp")
    m = Classification(class_type, size=(32, 64), channels_in=128, resize=256)
    m.load_state_dict(_round_weights(P32))
    m = m.cuda().train()
    xb = torch.from_numpy(x).cuda().to(torch.bfloat16)
    with torch.no_grad():
        y = m(xb)
    assert y.dtype == torch.float32
    pre = "%s_f64_" % class_type
    e_tr = _l2(y, gold[pre + "train_out"])
    m.eval()
    with torch.no_grad():
        ye = m(xb)
    e_ev = _l2(ye, gold[pre + "eval_out"])
    print("%s/%s head in bf16 vs the fp64 golden: train %.2e, eval %.2e (relative L2)" % (tree, class_type, e_tr, e_ev))
    assert e_tr < GOLDEN_BOUND and e_ev < GOLDEN_BOUND


def _bev_net(precision, P):
    from lanedetection_end2end_amd.bev.Networks import define_model
    net = define_model('erfnet', layers=18, in_channels=3, out_channels=2, pretrained=False, pool=True)
    net.load_state_dict(P)
    net = net.cuda()
    net.precision = precision
    return net


def _engine_state_bf16(net, ws, N, H, W):
    """The backbone's saved forward tensors in precision mode 2 (bf16 elements), keyed like the oracle's taps, plus the folded
    fp32 vectors of every non_bottleneck_1d's bn1 (as test_backbone_gpu.fetch_all reads them in the fp32 modes)."""
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    plan = net._plan(N, H, W)
    out, h, w = {}, H, W
    for li, (prefix, kind, cin, cout, _, _) in enumerate(erfnet_oracle.layer_table()):
        if kind == "down":
            h, w = h // 2, w // 2
        elif kind == "up":
            h, w = h * 2, w * 2
        nslots = {"down": 2, "nb1d": 5, "up": 2}[kind]
        for slot in range(nslots):
            key = prefix if slot == nslots - 1 else "%s#%d" % (prefix, slot)
            off, n = lib.lf_erfnet_activation_offset(plan.handle, li, slot), N * h * w * cout
            out[key] = ws.view(torch.bfloat16)[2 * off: 2 * off + n].view(N, h, w, cout).permute(0, 3, 1, 2).float().cpu()
        if kind == "nb1d":
            vec = []
            for which in (0, 1):
                off = lib.lf_erfnet_bn_vector_offset(plan.handle, li, 0, which)
                vec.append(ws.view(torch.float32)[off: off + cout].clone().cpu())
            out[prefix + "#bn1"] = tuple(vec)
    return out


def test_encoder_gradient_injection_bf16_eval():
    """loss = <enc, G> + <dec, Gd> in bf16, EVAL mode (affine BatchNorm backward: no chain of train-mode BatchNorm backwards
    amplifies the 2^-9 rounding): every parameter gradient against fp64 on the same bf16-rounded weights, evaluated
    straight-through at the engine's own forward state (its bf16 saved tensors and ReLU masks, as
    test_clas_gpu.test_encoder_output_gradient_injection does in fp32); and without the encoder term
    encoder.layers.14.conv1x3_2.weight's gradient moves.  Gates: per-channel gradients (conv biases, BatchNorm weights and biases)
    are sums over every pixel whose terms cancel -- the upstream gradient is uncorrelated with the activations here -- 2^-5;
    convolution weights 2^-6.  Measured on MI355X: per-channel 1.44e-2 (encoder.layers.4.bn1.weight), convolution weights
    1.32e-2 (encoder.layers.2.conv3x1_1.weight)."""
    N, H, W = 2, 64, 128
    P = _round_weights(erfnet_oracle.make_params(seed=3, out_channels=2))
    net = _bev_net("bf16", P).eval()
    x = torch.from_numpy(inputs.images(N, H, W, seed=51))
    rng = np.random.default_rng(9)
    G = torch.from_numpy(rng.standard_normal((N, 128, H // 8, W // 8)))
    Gd = torch.from_numpy(rng.standard_normal((N, 2, H, W)))
    enc, dec = net(x.cuda(), True)
    assert enc.dtype == torch.bfloat16 and enc.requires_grad
    state = _engine_state_bf16(net, dec.grad_fn.ws, N, H, W)
    ((enc.float() * G.float().cuda()).sum() + (dec * Gd.float().cuda()).sum()).backward()
    Pd = erfnet_oracle.cast_params(P, torch.float64)
    keys = [k for k, v in Pd.items() if v.is_floating_point() and "running" not in k]
    for k in keys:
        Pd[k].requires_grad_(True)
    eo, do = erfnet_oracle.erfnet_forward(x.double(), Pd, training=False, keep_masks=None, override=state)
    ((eo * G).sum() + (do * Gd).sum()).backward()
    worst = {"per-channel": (0.0, None), "conv weight": (0.0, None)}
    for k, p in net.named_parameters():
        ref = Pd[k].grad if k in Pd else None
        if ref is None or float(ref.abs().max()) == 0:
            assert p.grad is None or float(p.grad.abs().max()) == 0, k
            continue
        e = _l2(p.grad, ref)
        cls = "conv weight" if p.dim() == 4 else "per-channel"
        if e > worst[cls][0]:
            worst[cls] = (e, k)
    print("bf16 encoder-gradient injection (eval), worst parameter-gradient relative L2: per-channel %.2e at %s, "
          "convolution weights %.2e at %s" % (worst["per-channel"] + worst["conv weight"]))
    assert worst["per-channel"][0] < B5 and worst["conv weight"][0] < 2.0 ** -6, worst
    k = "encoder.layers.14.conv1x3_2.weight"
    net.zero_grad(set_to_none=True)
    enc, dec = net(x.cuda(), True)
    (dec * Gd.float().cuda()).sum().backward()
    assert _l2(dict(net.named_parameters())[k].grad, Pd[k].grad) > 0.1


def test_only_encode_bf16():
    """Net.forward(only_encode=True) in bf16 (refused before): output within 1e-2 relative L2 of the fp32 mode on the same
    rounded weights in eval mode; backward gives the encoder (and encoder.output_conv) gradients and the decoder none."""
    N, H, W = 2, 64, 128
    P = _round_weights(erfnet_oracle.make_params(seed=3, out_channels=2))
    x = torch.from_numpy(inputs.images(N, H, W, seed=52)).cuda()
    out = {}
    for precision in ("fp32", "bf16"):
        net = _bev_net(precision, P).eval()
        y = net(x, True, only_encode=True)
        assert y.dtype == torch.float32 and y.shape == (N, 2, H // 8, W // 8)
        out[precision] = y.detach()
        if precision == "bf16":
            y.square().sum().backward()
            for k, p in net.named_parameters():
                if k.startswith("decoder."):
                    assert p.grad is None, k
                else:
                    assert p.grad is not None and torch.isfinite(p.grad).all(), k
            assert float(net.encoder.layers[14].conv1x3_2.weight.grad.abs().max()) > 0
            assert float(net.encoder.output_conv.weight.grad.abs().max()) > 0
    e = _l2(out["bf16"], out["fp32"])
    print("only_encode bf16 vs fp32 (eval): relative L2 %.2e" % e)
    assert e < 1e-2


def test_encoder_output_is_a_differentiable_bf16_view():
    net = _bev_net("bf16", erfnet_oracle.make_params(seed=4, out_channels=2)).train()
    x = torch.rand(2, 3, 64, 128, device="cuda")
    enc, dec = net(x, True)
    assert enc.dtype == torch.bfloat16 and enc.requires_grad and enc.shape == (2, 128, 8, 16)
    assert enc.permute(0, 2, 3, 1).is_contiguous()
    enc.float().sum().backward()
    assert float(net.encoder.layers[14].conv1x3_2.weight.grad.abs().max()) > 0
    assert float(net.decoder.layers[0].conv.weight.grad.abs().max()) == 0


def test_bev_net_with_clas_heads_in_bf16():
    """The BEV tree's Net(clas=True) in bf16: line (N,3,4) / horizon fp32 logits, cross-entropy + BCE, gradients reach the
    encoder and every head parameter."""
    from argparse import Namespace
    from lanedetection_end2end_amd.bev.Loss_crit import Area_Loss
    from lanedetection_end2end_amd.bev.Networks.LSQ_layer import Net
    N, R = 2, 256
    args = Namespace(batch_size=N, nclasses=2, resize=R, end_to_end=True, mod="erfnet", layers=18, channels_in=3,
                     pretrained=False, pool=True, activation_layer="square", no_cuda=False, order=2, reg_ls=0.0,
                     use_cholesky=False, mask_percentage=0.3, clas=True, precision="bf16")
    model = Net(args)
    model.net.load_state_dict(erfnet_oracle.make_params(seed=5, out_channels=2))
    model = model.cuda().train()
    x = torch.from_numpy(inputs.images(N, R, 2 * R, seed=71)).cuda()
    gt = torch.from_numpy(inputs.bev_gt_params(N, seed=72)).cuda()
    rng = np.random.default_rng(5)
    gt_line = torch.from_numpy(rng.integers(0, 3, (N, 4))).cuda()
    gt_hor = torch.from_numpy((rng.uniform(0, 1, (N, R)) > 0.5).astype(np.float32)).cuda()
    b0, b1, _, _, _, _, _, line, horizon = model(x, True)
    assert line.shape == (N, 3, 4) and line.dtype == torch.float32 and horizon.dtype == torch.float32
    crit = Area_Loss(2, "none")
    loss = crit(b0, gt[:, 0]) + crit(b1, gt[:, 1]) + torch.nn.CrossEntropyLoss()(line, gt_line) + \
        torch.nn.BCEWithLogitsLoss()(horizon, gt_hor)
    loss.backward()
    assert torch.isfinite(loss)
    g = model.net.encoder.initial_block.conv.weight.grad
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    for k, p in model.named_parameters():
        if k.startswith(("line_classification.", "horizon_estimation.")):
            assert p.grad is not None and torch.isfinite(p.grad).all(), k


def _recipe_curve(precision, steps, N, R, K):
    from lanedetection_end2end_amd.bp.Loss_crit import backprojection_loss
    from lanedetection_end2end_amd.optim import FusedAdam
    model, args = _recipe_model(N, R, K, precision)
    crit = backprojection_loss(args)
    data = _recipe_data(N, R, K, seed=171)
    params = list(model.parameters())
    opt = FusedAdam(params, lr=1e-4)
    curve = []
    for _ in range(steps):
        loss, _, _ = _recipe_loss(model, args, crit, data)
        for p in params:
            p.grad = None
        loss.backward()
        opt.step()
        curve.append(float(loss))
    return np.asarray(curve)


def test_recipe_bf16_training_tracks_fp32():
    """40 FusedAdam steps of the train.sh recipe (fit + line + horizon losses) at 4 x 256 x 512 from the same weights: the mean of
    the last ten losses in bf16 within 5 % of fp32's (as test_c3_bf16_training_tracks_fp32 does for the heads-free model)."""
    N, R, K, steps = 4, 256, 4, 40
    curves = {m: _recipe_curve(m, steps, N, R, K) for m in ("fp32", "bf16")}
    for m, c in curves.items():
        print("%-5s recipe loss: first %.4f  steps 10/20/30 %.4f %.4f %.4f  mean of last ten %.4f" % (
            m, c[0], c[10], c[20], c[30], c[-10:].mean()))
        assert np.isfinite(c).all(), m
        assert c[-10:].mean() < c[:3].mean(), (m, "loss did not fall")
    ref, got = curves["fp32"][-10:].mean(), curves["bf16"][-10:].mean()
    assert abs(got - ref) <= 0.05 * ref, (got, ref)
