"""Input-image gradient on the GPU: the stem's data-gradient kernel through the C ABI (``lf_stem_bwd_data``) against the fp64
restatement in tests/input_grad_ref.py, its footprints, and ``input.grad`` through every surface that reaches the stem -- the whole
network in the three precision modes, train and eval BatchNorm, both heads, ``only_encode``, the encoder output joining the
logits, the block-level calls, and the BEV / BP ``Net`` mirrors -- against the fp64 oracle evaluated straight-through at the
engine's own forward state (the protocol of tests/test_baseline_configs_gpu.py::_check_grads_straight_through).

Gates.  Kernel: |gimg - R| <= 64 * 2^-24 * S + 1e-37 per element, S = sum |w| |g| + |g_pool| (an fp32 sum of at most 4 * 15 + 1 = 61
exact-input products: the standard (n + 1) u sum |terms| bound).  Whole network, fp32 and fp32x9: |x.grad - g64| <= 3e-5 * max |g64|,
the gate that protocol holds every parameter gradient to (the image gradient is a 61-term sum of the same gcat that
initial_block.conv.weight's gradient sums over all pixels).  bf16: relative L2 < 0.25, the gate
tests/test_backbone_gpu.py::test_bf16_tensor_mode_backward_straight_through holds the worst (= the stem's) parameter gradient to."""
import ctypes
from argparse import Namespace

import numpy as np
import pytest
import torch

import synthetic_inputs
from input_grad_ref import input_grad_ref
from oracle import erfnet_oracle

pytestmark = pytest.mark.gpu

GUARD = 256
SENTINEL = -12345.5
SHAPES = [(2, 3, 6, 32), (1, 1, 4, 64), (2, 4, 16, 32), (1, 3, 10, 18), (3, 3, 34, 30)]
TOL_NET = 3e-5
TOL_BF16_L2 = 0.25


# ---- the kernel through the C ABI -------------------------------------------------------------------------------------------

def _kernel_inputs(shape, s16, seed):
    N, Cin, H, W = shape
    rng = np.random.default_rng(1000 + seed)
    img = torch.from_numpy(synthetic_inputs.images(N, H, W, seed=seed, C=Cin))
    gcat = torch.from_numpy(rng.standard_normal((N, H // 2, W // 2, 16)).astype(np.float32))
    if s16:
        gcat = gcat.bfloat16().float()                      # rounded first: the stored values ARE the reference's inputs
    w = torch.from_numpy(rng.standard_normal((16 - Cin, Cin, 3, 3)).astype(np.float32) * 0.3)
    return gcat, img, w


def _launch(gcat, img, w, s16):
    """gimg inside a larger buffer, GUARD sentinel floats on each side; returns (gimg clone, guards untouched)."""
    from lanedetection_end2end_amd import _lib
    lib = _lib.load()
    N, Cin, H, W = img.shape
    n = img.numel()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    g = (gcat.bfloat16() if s16 else gcat).cuda().contiguous()
    xi, wd = img.cuda().contiguous(), w.cuda().contiguous()
    out = buf[GUARD: GUARD + n]
    _lib.check(lib.lf_stem_bwd_data(ctypes.c_void_p(g.data_ptr()), _lib.ptr(xi), _lib.ptr(wd), N, Cin, H, W, int(s16),
                                    ctypes.c_void_p(out.data_ptr()), _lib.stream()), "lf_stem_bwd_data")
    torch.cuda.synchronize()
    guards_ok = bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())
    return out.clone().view(N, Cin, H, W), guards_ok


@pytest.mark.parametrize("s16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,seed", list(zip(SHAPES, range(31, 36))), ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernel_against_the_reference(shape, seed, s16):
    gcat, img, w = _kernel_inputs(shape, s16, seed)
    got, guards_ok = _launch(gcat, img, w, s16)
    R, S = input_grad_ref(gcat.numpy(), img.numpy(), w.numpy())
    d = np.abs(got.cpu().double().numpy() - R)
    bound = 64 * 2.0 ** -24 * S + 1e-37
    print("%s %s: worst |gimg - R| / (2^-24 S) = %.2f (gate 64), max |R| %.2f" % (shape, "bf16" if s16 else "fp32",
                                                                                 float((d / (2.0 ** -24 * S)).max()), np.abs(R).max()))
    assert guards_ok, "a guard float around gimg was overwritten"
    assert not bool((got == SENTINEL).any()), "an element of gimg was not written"
    assert np.all(d <= bound), (float((d / bound).max()), np.argwhere(d > bound)[:5])
    again, guards_ok = _launch(gcat, img, w, s16)
    assert guards_ok and torch.equal(again, got)             # the same bits on every launch


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("s16", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_footprints(value, s16):
    """One non-finite element of gcat reaches exactly the image pixels the formula names, nothing else changes by a bit."""
    shape = (2, 3, 6, 32)
    N, Cin, H, W = shape
    Cc, Ho, Wo = 16 - Cin, H // 2, W // 2
    gcat, img, w = _kernel_inputs(shape, s16, 31)
    clean, _ = _launch(gcat, img, w, s16)
    assert torch.isfinite(clean).all()
    # convolution channels: corner, top edge, left edge, right edge, bottom-right corner, interior
    for (n, oy, ox, co) in [(0, 0, 0, 0), (1, 0, 7, 5), (0, 1, 0, Cc - 1), (1, 1, Wo - 1, 3), (0, Ho - 1, Wo - 1, 12), (1, 1, 9, 7)]:
        g = gcat.clone()
        g[n, oy, ox, co] = value
        got, guards_ok = _launch(g, img, w, s16)
        hit = torch.zeros(shape, dtype=torch.bool)
        hit[n, :, max(2 * oy - 1, 0): 2 * oy + 2, max(2 * ox - 1, 0): 2 * ox + 2] = True      # clipped to the image; every channel
        got = got.cpu()
        assert guards_ok
        assert torch.equal(~torch.isfinite(got), hit), (n, oy, ox, co)
        if value != value:
            assert torch.isnan(got[hit]).all()
        assert _same_bits(got[~hit], clean.cpu()[~hit]), (n, oy, ox, co)
    # pooled channels: the window's arg-max pixel of that image channel, and only it
    for (n, oy, ox, ci) in [(0, 0, 0, 0), (1, 2, 15, 2), (0, 1, 4, 1), (1, 0, 11, 2)]:
        g = gcat.clone()
        g[n, oy, ox, Cc + ci] = value
        got, guards_ok = _launch(g, img, w, s16)
        win = img[n, ci, 2 * oy: 2 * oy + 2, 2 * ox: 2 * ox + 2].reshape(-1)
        j = int(torch.argmax(win))                                                            # (no ties in these images)
        assert int((win == win[j]).sum()) == 1
        hit = torch.zeros(shape, dtype=torch.bool)
        hit[n, ci, 2 * oy + (j >> 1), 2 * ox + (j & 1)] = True
        got = got.cpu()
        assert guards_ok
        assert torch.equal(~torch.isfinite(got), hit), (n, oy, ox, ci)
        assert _same_bits(got[~hit], clean.cpu()[~hit]), (n, oy, ox, ci)


# ---- the whole network ------------------------------------------------------------------------------------------------------

def _build(out_channels=2, seed=3, pretrained=False, dropout=True):
    from test_backbone_gpu import build
    net, P = build(out_channels=out_channels, seed=seed, pretrained=pretrained)
    if not dropout:
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout2d):
                m.p = 0
    return net, P


def _spy_masks(net):
    """Record the Dropout2d keep-masks the module draws (as tests/test_backbone_gpu.py::test_dropout_masks_and_pretrained_head)."""
    drawn = {}
    orig = net._make_dropmask

    def spy(plan, device):
        m = orig(plan, device)
        if m is not None:
            drawn["mask"], drawn["plan"] = m.clone(), plan
        return m
    net._make_dropmask = spy
    return drawn


def _keep_of(drawn, N):
    if "mask" not in drawn:
        return None
    plan, mask = drawn["plan"], drawn["mask"].cpu()
    blocks = [p for p, kind, _, _, dp, _ in erfnet_oracle.layer_table() if kind == "nb1d" and dp > 0]
    return {prefix: mask[off: off + N * ch].view(N, ch) for prefix, off, ch in zip(blocks, plan.drop_off, plan.drop_ch)}


def _oracle_xgrad(x, P, state, keep, training, head, loss_of):
    """d loss / d x of the oracle evaluated straight-through at the engine's forward state, in fp64 and fp32.
    loss_of(enc, dec, Pd, dtype) -> the scalar the engine's backward was driven by."""
    out = {}
    for dt in (torch.float64, torch.float32):
        Pd = erfnet_oracle.cast_params(P, dt)
        xd = x.detach().cpu().to(dt).requires_grad_(True)
        enc, dec = erfnet_oracle.erfnet_forward(xd, Pd, training=training, keep_masks=keep, head=head, override=state)
        loss_of(enc, dec, Pd, dt).backward()
        out[dt] = xd.grad.double()
    return out[torch.float64], out[torch.float32]


def _gate(name, got, g64, g32, tol=TOL_NET):
    got = got.detach().cpu().double()
    scale = float(g64.abs().max())
    e, fl = float((got - g64).abs().max()) / scale, float((g32 - g64).abs().max()) / scale
    print("%-44s |x.grad - g64| %.2e   |cpu32 - g64| %.2e   (of max |g64| = %.3e; gate %.0e)" % (name, e, fl, scale, tol))
    assert scale > 0 and torch.isfinite(got).all()
    assert e <= tol, (name, e, fl)


def _whole_network(precision, N, H, W, training, seed):
    from test_backbone_gpu import fetch_all
    net, P = _build(seed=seed)
    net.train(training)
    net.precision = precision
    drawn = _spy_masks(net)
    x = torch.from_numpy(synthetic_inputs.images(N, H, W, seed=seed + 40)).cuda().requires_grad_(True)
    gy = torch.from_numpy(np.random.default_rng(seed + 41).standard_normal((N, 2, H, W)).astype(np.float32))
    torch.manual_seed(seed)
    enc, dec = net(x, True)
    state = fetch_all(net, net._plan(N, H, W), dec.grad_fn.ws, N, H, W)
    (dec * gy.cuda()).sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape
    g64, g32 = _oracle_xgrad(x, P, state, _keep_of(drawn, N) if training else None, training, "output_conv",
                             lambda e, d, Pd, dt: (d * gy.to(dt)).sum())
    _gate("%s %dx3x%dx%d train=%d" % (precision, N, H, W, training), x.grad, g64, g32)


@pytest.mark.parametrize("precision", ["fp32", "fp32x9"])
@pytest.mark.parametrize("N,H,W", [(2, 32, 64), (1, 48, 96)])
def test_whole_network_train_mode_with_dropout(precision, N, H, W):
    _whole_network(precision, N, H, W, True, seed=5)


@pytest.mark.parametrize("precision", ["fp32", "fp32x9"])
def test_whole_network_eval_mode(precision):
    _whole_network(precision, 2, 32, 64, False, seed=6)


# ---- surfaces ---------------------------------------------------------------------------------------------------------------

def _backbone_node(t):
    """The autograd node of the backbone Function (it holds the workspace) below tensor t."""
    seen, todo = set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if hasattr(fn, "ws") and fn.ws is not None:
            return fn
        todo += [f for f, _ in fn.next_functions]
    raise AssertionError("no backbone node below the tensor")


def test_only_encode():
    from test_backbone_gpu import fetch_all
    N, H, W = 2, 32, 64
    net, P = _build(seed=7, dropout=False)
    net.train()
    x = torch.from_numpy(synthetic_inputs.images(N, H, W, seed=47)).cuda().requires_grad_(True)
    y = net(x, True, only_encode=True)
    gy = torch.from_numpy(np.random.default_rng(48).standard_normal(tuple(y.shape)).astype(np.float32))
    state = fetch_all(net, net._plan(N, H, W), _backbone_node(y).ws, N, H, W)
    state = {k: v for k, v in state.items() if k.startswith("encoder.")}          # (the decoder did not run)
    (y * gy.cuda()).sum().backward()

    def loss_of(enc, dec, Pd, dt):
        return (torch.nn.functional.conv2d(enc, Pd["encoder.output_conv.weight"], Pd["encoder.output_conv.bias"]) * gy.to(dt)).sum()
    g64, g32 = _oracle_xgrad(x, P, state, None, True, "output_conv", loss_of)
    _gate("only_encode (head -1)", x.grad, g64, g32)


def test_logits_and_encoder_output_join():
    from test_backbone_gpu import fetch_all
    N, H, W = 2, 32, 64
    net, P = _build(seed=8, dropout=False)
    net.train()
    x = torch.from_numpy(synthetic_inputs.images(N, H, W, seed=49)).cuda().requires_grad_(True)
    rng = np.random.default_rng(50)
    gy = torch.from_numpy(rng.standard_normal((N, 2, H, W)).astype(np.float32))
    ge = torch.from_numpy(rng.standard_normal((N, 128, H // 8, W // 8)).astype(np.float32))
    enc, dec = net(x, True)
    state = fetch_all(net, net._plan(N, H, W), dec.grad_fn.ws, N, H, W)
    ((dec * gy.cuda()).sum() + (enc * ge.cuda()).sum()).backward()
    g64, g32 = _oracle_xgrad(x, P, state, None, True, "output_conv",
                             lambda e, d, Pd, dt: (d * gy.to(dt)).sum() + (e * ge.to(dt)).sum())
    _gate("logits + encoder output (grad_encoder)", x.grad, g64, g32)
    # the encoder output alone moves the image too
    x2 = x.detach().clone().requires_grad_(True)
    enc2, _ = net(x2, True)
    (enc2 * ge.cuda()).sum().backward()
    assert float(x2.grad.abs().max()) > 0 and not torch.equal(x2.grad, x.grad)


def test_pretrained_second_head():
    from test_backbone_gpu import fetch_all
    N, H, W = 2, 32, 64
    net, P = _build(seed=9, pretrained=True, dropout=False)
    net.train()
    x = torch.from_numpy(synthetic_inputs.images(N, H, W, seed=51)).cuda().requires_grad_(True)
    gy = torch.from_numpy(np.random.default_rng(52).standard_normal((N, 3, H, W)).astype(np.float32))
    enc, dec = net(x, False)                        # flag False + pretrained: output_conv2 (head 1)
    assert dec.shape == (N, 3, H, W)
    state = fetch_all(net, net._plan(N, H, W), dec.grad_fn.ws, N, H, W)
    (dec * gy.cuda()).sum().backward()
    g64, g32 = _oracle_xgrad(x, P, state, None, True, "output_conv2", lambda e, d, Pd, dt: (d * gy.to(dt)).sum())
    _gate("pretrained, flag False (head 1)", x.grad, g64, g32)


def test_initial_block_alone():
    """net.encoder.initial_block(x): layer range [0, 1).  Reference: tests/input_grad_ref.py on the gradient of the concat
    buffer, which torch computes in fp64 through train-mode BatchNorm (eps 1e-3) and the ReLU -- the ReLU's derivative mask is the
    engine's own output > 0, as in the straight-through protocol."""
    N, H, W = 2, 32, 64
    net, P = _build(seed=10, dropout=False)
    net.train()
    x = torch.from_numpy(synthetic_inputs.images(N, H, W, seed=53))
    xg = x.cuda().requires_grad_(True)
    y = net.encoder.initial_block(xg)
    assert y.shape == (N, 16, H // 2, W // 2)
    gy = torch.from_numpy(np.random.default_rng(54).standard_normal(tuple(y.shape)).astype(np.float32))
    (y * gy.cuda()).sum().backward()
    assert xg.grad is not None
    refs = {}
    for dt in (torch.float64, torch.float32):
        Pd = erfnet_oracle.cast_params(P, dt)
        w, b = Pd["encoder.initial_block.conv.weight"], Pd["encoder.initial_block.conv.bias"]
        cat = torch.cat([torch.nn.functional.conv2d(x.to(dt), w, b, stride=2, padding=1), torch.nn.functional.max_pool2d(x.to(dt), 2)], 1)
        cat = cat.detach().requires_grad_(True)
        z = torch.nn.functional.batch_norm(cat, None, None, Pd["encoder.initial_block.bn.weight"], Pd["encoder.initial_block.bn.bias"],
                                           True, 0.1, erfnet_oracle.BN_EPS)
        ((z * (y.detach().cpu() > 0).to(dt)) * gy.to(dt)).sum().backward()
        refs[dt] = torch.from_numpy(input_grad_ref(cat.grad.permute(0, 2, 3, 1).double().numpy(), x.double().numpy(), w.double().numpy())[0])
    _gate("encoder.initial_block(x) (range [0, 1))", xg.grad, refs[torch.float64], refs[torch.float32])
    others = [k for k, p in net.named_parameters() if not k.startswith("encoder.initial_block.") and p.grad is not None]
    assert not others, others


def test_encoder_alone():
    """net.encoder(x): layer range [0, 16).  Its activations are the whole network's bit for bit
    (tests/test_blocks_gpu.py::test_encoder_and_decoder_compose_to_the_network), so the forward state of a whole-network run on
    the same input serves the straight-through oracle."""
    from test_backbone_gpu import fetch_all
    N, H, W = 2, 32, 64
    net, P = _build(seed=11, dropout=False)
    net.train()
    x = torch.from_numpy(synthetic_inputs.images(N, H, W, seed=55)).cuda()
    enc_f, dec_f = net(x, True)
    state = fetch_all(net, net._plan(N, H, W), dec_f.grad_fn.ws, N, H, W)
    state = {k: v for k, v in state.items() if k.startswith("encoder.")}
    xg = x.clone().requires_grad_(True)
    enc = net.encoder(xg)
    assert torch.equal(enc, enc_f.contiguous())
    ge = torch.from_numpy(np.random.default_rng(56).standard_normal(tuple(enc.shape)).astype(np.float32))
    (enc * ge.cuda()).sum().backward()
    g64, g32 = _oracle_xgrad(xg, P, state, None, True, "output_conv", lambda e, d, Pd, dt: (e * ge.to(dt)).sum())
    _gate("encoder(x) (range [0, 16))", xg.grad, g64, g32)


# ---- nothing changes when the gradient is not asked for ------------------------------------------------------------------------

def test_default_path_is_unchanged_and_frozen_stem():
    N, H, W = 2, 32, 64
    net, P = _build(seed=12)
    net.train()
    x = torch.from_numpy(synthetic_inputs.images(N, H, W, seed=57)).cuda()
    gy = torch.from_numpy(np.random.default_rng(58).standard_normal((N, 2, H, W)).astype(np.float32)).cuda()
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}

    def run(requires_grad):
        net.load_state_dict(sd0)
        for p in net.parameters():
            p.grad = None
        xi = x.clone().requires_grad_(requires_grad)
        torch.manual_seed(3)                         # the same Dropout2d masks
        enc, dec = net(xi, True)
        (dec * gy).sum().backward()
        return xi.grad, dec.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    gx0, dec0, g0 = run(False)
    gx1, dec1, g1 = run(True)
    assert gx0 is None
    assert gx1 is not None and torch.isfinite(gx1).all() and float(gx1.abs().max()) > 0
    assert torch.equal(dec0, dec1)
    assert sorted(g0) == sorted(g1) and "encoder.initial_block.conv.weight" in g1
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    # a frozen stem convolution takes no gradient; the image still does, and the same one
    net.encoder.initial_block.conv.weight.requires_grad_(False)
    net.encoder.initial_block.conv.bias.requires_grad_(False)
    gx2, dec2, g2 = run(True)
    assert "encoder.initial_block.conv.weight" not in g2 and "encoder.initial_block.conv.bias" not in g2
    assert gx2 is not None and torch.equal(gx2, gx1)
    for k in g2:
        assert torch.equal(g2[k], g1[k]), k


# ---- bf16 -------------------------------------------------------------------------------------------------------------------

def test_bf16_whole_network():
    """Precision mode "bf16" at 2 x 3 x 32 x 64: x.grad finite, and its relative L2 against the fp64 oracle evaluated straight-through
    at the engine's own (bf16-stored) forward state within the gate the bf16 whole-network test holds the stem's parameter
    gradients to (the image gradient sits at the end of exactly that chain of rounded gradient tensors)."""
    from lanedetection_end2end_amd import _lib
    N, H, W = 2, 32, 64
    net, P = _build(seed=3, dropout=False)
    net.train()
    net.precision = "bf16"
    x = torch.from_numpy(synthetic_inputs.images(N, H, W, seed=59)).cuda().requires_grad_(True)
    gy = torch.from_numpy(np.random.default_rng(60).standard_normal((N, 2, H, W)).astype(np.float32))
    enc, dec = net(x, True)
    plan, ws = net._plan(N, H, W), dec.grad_fn.ws
    lib = _lib.load()
    state, h, w = {}, H, W
    for li, (prefix, kind, cin, cout, _, _) in enumerate(erfnet_oracle.layer_table()):
        if kind == "down":
            h, w = h // 2, w // 2
        elif kind == "up":
            h, w = h * 2, w * 2
        nslots = {"down": 2, "nb1d": 5, "up": 2}[kind]
        for slot in range(nslots):
            off = lib.lf_erfnet_activation_offset(plan.handle, li, slot)
            t = ws.view(torch.bfloat16)[2 * off: 2 * off + N * h * w * cout].view(N, h, w, cout).permute(0, 3, 1, 2).float().cpu()
            state[prefix if slot == nslots - 1 else "%s#%d" % (prefix, slot)] = t
    (dec * gy.cuda()).sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    Pd = erfnet_oracle.cast_params(P, torch.float64)
    xd = x.detach().cpu().double().requires_grad_(True)
    _, dec_st = erfnet_oracle.erfnet_forward(xd, Pd, training=True, override=state)
    (dec_st * gy.double()).sum().backward()
    g = x.grad.cpu().double()
    err = float((g - xd.grad).norm() / xd.grad.norm())
    cos = float((g * xd.grad).sum() / (g.norm() * xd.grad.norm()))
    print("bf16 2x3x32x64: x.grad vs the straight-through fp64 oracle, relative L2 %.3e, cosine %.5f (gate %.2f)" % (err, cos, TOL_BF16_L2))
    assert err < TOL_BF16_L2


# ---- the BEV / BP mirrors -----------------------------------------------------------------------------------------------------

def _mirror_args(N, R, K, tree, order, clas):
    return Namespace(batch_size=N, nclasses=K, resize=R, end_to_end=True, mod="erfnet", layers=18, channels_in=3,
                     pretrained=False, pool=True, activation_layer="square", no_cuda=False, order=order, reg_ls=0.0,
                     use_cholesky=False, mask_percentage=0.3 if tree == "bev" else 0.2, clas=clas, no_mapping=False,
                     loss_policy="area" if tree == "bev" else "backproject", weight_seg=30, weight_funct="none")


def _mirror(model, forward_and_loss, x):
    """input.requires_grad_() -> forward -> criterion -> backward on a mirror; then the same d loss / d logits (and d loss / d encoder
    output) fed into the backbone alone: the same bits in input.grad."""
    model = model.cuda()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0
    model.train()
    grabbed = {}

    def grab(mod, inp, out):
        grabbed["enc"], grabbed["dec"] = out[0], out[1]
        if out[0].requires_grad:                     # (a model without the --clas heads does not export the encoder output)
            out[0].retain_grad()
        out[1].retain_grad()
    hook = model.net.register_forward_hook(grab)
    sd0 = {k: v.clone() for k, v in model.net.state_dict().items()}
    xi = x.clone().requires_grad_(True)
    loss = forward_and_loss(model, xi)
    hook.remove()
    loss.backward()
    assert xi.grad is not None and torch.isfinite(xi.grad).all() and float(xi.grad.abs().max()) > 0
    enc, dec = grabbed["enc"], grabbed["dec"]
    assert dec.grad is not None
    model.net.load_state_dict(sd0)
    x2 = x.clone().requires_grad_(True)
    out = model.net(x2, True * model.pretrained)
    tensors, grads = [out[1]], [dec.grad]
    if enc.grad is not None:
        tensors.append(out[0])
        grads.append(enc.grad)
    torch.autograd.backward(tensors, grads)
    assert torch.equal(x2.grad, xi.grad)
    return enc.grad is not None


def test_bev_mirror():
    from lanedetection_end2end_amd.bev.Loss_crit import Area_Loss
    from lanedetection_end2end_amd.bev.Networks.LSQ_layer import Net
    N, R = 2, 256
    model = Net(_mirror_args(N, R, 2, "bev", 2, False))
    model.net.load_state_dict(erfnet_oracle.make_params(seed=4, out_channels=2))
    gt = torch.from_numpy(synthetic_inputs.bev_gt_params(N, seed=62)).cuda()
    crit = Area_Loss(2, "none")

    def step(model, xi):
        b0, b1 = model(xi, True)[:2]
        return crit(b0, gt[:, 0]) + crit(b1, gt[:, 1])
    _mirror(model, step, torch.from_numpy(synthetic_inputs.images(N, R, 2 * R, seed=61)).cuda())


def test_bp_mirror_with_clas_heads():
    from lanedetection_end2end_amd.bp.Loss_crit import backprojection_loss
    from lanedetection_end2end_amd.bp.Networks.LSQ_layer import Net
    N, R, K = 2, 256, 4
    args = _mirror_args(N, R, K, "bp", 3, True)
    model = Net(args)
    model.net.load_state_dict(erfnet_oracle.make_params(seed=5, out_channels=K))
    lanes, valid = synthetic_inputs.bp_targets(N, K, R, seed=64)
    crit = backprojection_loss(args)
    rng = np.random.default_rng(65)
    gt_line = torch.from_numpy((rng.uniform(0, 1, (N, 4)) > 0.5).astype(np.float32)).cuda()
    gt_hor = torch.from_numpy((rng.uniform(0, 1, (N, R)) > 0.5).astype(np.float32)).cuda()
    bce = torch.nn.BCEWithLogitsLoss()

    def step(model, xi):
        out = model(xi, torch.zeros(N, K), True)
        loss = (bce(out[6], gt_line) + bce(out[7], gt_hor)).double()
        for k in range(K):
            loss = loss + crit(out[k], torch.from_numpy(lanes[:, k]).cuda(), torch.from_numpy(valid[:, k]).cuda())[0] / K
        return loss
    joined = _mirror(model, step, torch.from_numpy(synthetic_inputs.images(N, R, 2 * R, seed=63)).cuda())
    assert joined                                    # the --clas heads sent a gradient into the encoder output
