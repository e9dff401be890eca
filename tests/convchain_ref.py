"""Plain-torch reference of a chain of [Conv2d(k x k, stride 1, pad k / 2, bias) -> BatchNorm2d -> ReLU] blocks (csrc/lf_convchain.hip),
for any channel counts and any kernel sizes in {1, 3}.  Every function takes the dtype it computes in: torch.float64 is the reference,
torch.float32 the same arithmetic with torch's fp32 CPU operators on the same operands -- the error scale the fp32 kernels are held to
(tests/test_convchain_shapes_gpu.py).  Tensors are NCHW on the CPU.

  params   4 per block, module order: conv.weight (Co,Ci,k,k), conv.bias, bn.weight, bn.bias
  running  2 per block: running_mean, running_var
  state    per block (z, sc, sh): the pre-BatchNorm tensor and the folded scale / shift a forward left behind -- the engine's own
           (its stored z, bf16 in precision mode 2, and its fp32 vectors), or forward_free's

Teacher forcing: block i's reference convolution reads a_{i-1} = relu(z_{i-1} * sc + sh) formed from the STATE, so a block is compared
on the operand the engine itself read and no ReLU decision is ever compared across precisions.  The straight-through backward gives
every z the state's value with the convolution's own derivative and every ReLU the state's mask, z * sc + sh > 0: what is left to
differ is backward arithmetic.  (tests/test_convchain_ref_cpu.py checks these against plain autograd.)"""
import torch
import torch.nn.functional as F

MOMENTUM, EPS = 0.1, 1e-5


def cast(ts, dtype):
    return [t.detach().to(dtype) for t in ts]


def _c(v):
    return v[None, :, None, None]


def conv(a, w, b):
    return F.conv2d(a, w, b, padding=(w.shape[2] - 1) // 2)


def operand(x, state, i, dtype):
    """What block i's convolution reads: x for block 0, else relu(z * sc + sh) of block i - 1's state."""
    if i == 0:
        return x.to(dtype)
    z, sc, sh = (t.to(dtype) for t in state[i - 1][:3])
    return torch.relu(z * _c(sc) + _c(sh))


def forward_teacher(x, params, state, dtype=torch.float64):
    """-> [z_ref_i]: conv(a_{i-1}) + b with a_{i-1} from the state."""
    p = cast(params, dtype)
    return [conv(operand(x, state, i, dtype), p[4 * i], p[4 * i + 1]) for i in range(len(params) // 4)]


def bn_vectors(z, gamma, beta, rmean, rvar, training, momentum=MOMENTUM, eps=EPS, dtype=torch.float64):
    """The BatchNorm vectors of one block from its pre-BN tensor z (train mode: batch statistics, biased variance; running statistics
    updated with the unbiased one) or from the running statistics (eval mode, which leaves them alone).
    -> dict: mean, var (the ones normalised with), sc = gamma * rstd, sh = beta - mean * sc, asc = rstd, ash = -mean * rstd, rmean, rvar."""
    z, gamma, beta, rmean, rvar = (t.to(dtype) for t in (z, gamma, beta, rmean, rvar))
    o = {}
    if training:
        count = z.numel() // z.shape[1]
        mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        unb = var * count / (count - 1.0) if count > 1 else var
        o["rmean"], o["rvar"] = (1 - momentum) * rmean + momentum * mean, (1 - momentum) * rvar + momentum * unb
    else:
        mean, var = rmean, rvar
        o["rmean"], o["rvar"] = rmean, rvar
    rstd = 1.0 / torch.sqrt(var + eps)
    o.update(mean=mean, var=var, asc=rstd, ash=-mean * rstd, sc=gamma * rstd, sh=beta - mean * gamma * rstd)
    return o


def forward_free(x, params, running, training, momentum=MOMENTUM, eps=EPS, dtype=torch.float64):
    """The chain run on its own: -> (y, state, new running statistics)."""
    p, r = cast(params, dtype), cast(running, dtype)
    a, state, new_running = x.to(dtype), [], []
    for i in range(len(p) // 4):
        z = conv(a, p[4 * i], p[4 * i + 1])
        v = bn_vectors(z, p[4 * i + 2], p[4 * i + 3], r[2 * i], r[2 * i + 1], training, momentum, eps, dtype)
        state.append((z, v["sc"], v["sh"]))
        new_running += [v["rmean"], v["rvar"]]
        a = torch.relu(z * _c(v["sc"]) + _c(v["sh"]))
    return a, state, new_running


def output(state, dtype=torch.float64):
    """y = relu(z_L * sc + sh) of the last block's state."""
    return operand(None, state, len(state), dtype)


def straight_through(x, params, running, state, training, eps=EPS, dtype=torch.float64):
    """The chain as an autograd graph evaluated at the state: z_i takes the state's VALUE and keeps conv's derivative, BatchNorm is
    torch's formula on that z (train mode: its own batch statistics, differentiated through; eval mode: the running statistics), every
    ReLU is the state's mask.  x and params must be leaves of `dtype` that require grad.  -> (y, [z_i]) with z_i.retain_grad() set."""
    a, zs = x, []
    for i in range(len(params) // 4):
        w, b, gamma, beta = params[4 * i: 4 * i + 4]
        ze, sc, sh = (t.detach().to(dtype) for t in state[i][:3])
        z = conv(a, w, b)
        z = z + (ze - z).detach()
        z.retain_grad()
        zs.append(z)
        if training:
            mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
        else:
            mean, var = running[2 * i].detach().to(dtype), running[2 * i + 1].detach().to(dtype)
        h = (z - _c(mean)) / torch.sqrt(_c(var) + eps) * _c(gamma) + _c(beta)
        a = h * ((ze * _c(sc) + _c(sh)) > 0).to(dtype)
    return a, zs


def backward_straight_through(x, gy, params, running, state, training, eps=EPS, dtype=torch.float64):
    """-> (gx, [4L parameter gradients], [d loss / d z_i]) of <y, gy> straight-through at the state."""
    xl = x.detach().to(dtype).requires_grad_(True)
    pl = [t.requires_grad_(True) for t in cast(params, dtype)]
    y, zs = straight_through(xl, pl, running, state, training, eps, dtype)
    (y * gy.to(dtype)).sum().backward()
    return xl.grad, [t.grad for t in pl], [z.grad for z in zs]


def folded(x, params, running, eps=EPS, dtype=torch.float64):
    """Inference form: relu(conv(x, w * s) + (b - mean) * s + beta) per block, s = gamma / sqrt(var + eps)."""
    p, r = cast(params, dtype), cast(running, dtype)
    a = x.to(dtype)
    for i in range(len(p) // 4):
        w, b, gamma, beta = p[4 * i: 4 * i + 4]
        s = gamma / torch.sqrt(r[2 * i + 1] + eps)
        a = torch.relu(conv(a, w * s[:, None, None, None], (b - r[2 * i]) * s + beta))
    return a


def relmax(got, ref):
    """The project's fp32 metric: max |got - ref| / max |ref|."""
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def rell2(got, ref):
    got, ref = got.detach().double(), ref.detach().double()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))
