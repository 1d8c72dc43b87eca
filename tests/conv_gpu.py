"""GPU side of the convolution-stack oracle: runs one case of tests/conv_oracle.py through the C entry points of csrc/conv.hip with
every output buffer -- the statistics workspace included -- holding NaN (0xFF bytes for the arg-max taps) beforehand, and returns the
outputs under the oracle's names.  The entry points are called through lib().call, not through the kernels.py wrappers, so that the test
owns every buffer."""
import torch

from ofasys_amd import lib as L
from tests import conv_oracle as co

DEV = "cuda"
NAN = float("nan")
F32 = torch.float32
CODE = {co.F32: L.F32, co.BF16: L.BF16, co.FP16: L.F16}


def nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _call(name, *args):
    L.lib().call(name, *[L.ptr(a) if torch.is_tensor(a) else a for a in args], L.stream())
    torch.cuda.synchronize()


def ws_for(C):
    return nan((L.lib().cdll.ofa_batchnorm_ws_floats(C),), F32)


def run_im2col(x, g, nchw):
    Ho, Wo = co.geom_out(g)
    col = nan((g.B * Ho * Wo, co.kpad(g)), x.dtype)
    _call("ofa_im2col", x, col, g.B, g.H, g.W, g.C, g.kh, g.kw, g.s, g.p, co.kpad(g), int(nchw), CODE[x.dtype])
    return col


def run_col2im(dcol, g):
    dx = nan((g.B * g.H * g.W, g.C), dcol.dtype)
    _call("ofa_col2im", dcol, dx, g.B, g.H, g.W, g.C, g.kh, g.kw, g.s, g.p, dcol.shape[1], CODE[dcol.dtype])
    return dx


def run_maxpool(x, g):
    Ho, Wo = co.geom_out(g)
    y = nan((g.B * Ho * Wo, g.C), x.dtype)
    arg = torch.full((g.B * Ho * Wo, g.C), 255, dtype=torch.uint8, device=DEV)
    _call("ofa_maxpool_fwd", x, y, arg, g.B, g.H, g.W, g.C, g.kh, g.s, g.p, CODE[x.dtype])
    return y, arg


def run_maxpool_bwd(dy, arg, g):
    dx = nan((g.B * g.H * g.W, g.C), dy.dtype)
    _call("ofa_maxpool_bwd", dy, arg, dx, g.B, g.H, g.W, g.C, g.kh, g.s, g.p, CODE[dy.dtype])
    return dx


def run_relu(x, gate=None):
    y = nan(x.shape, x.dtype)
    _call("ofa_relu", x, gate, y, x.numel(), CODE[x.dtype])
    return y


def _grads(c, C, dtype):
    if c["prev"] is not None:
        return c["prev"][0].clone(), c["prev"][1].clone(), 1
    return nan((C,), dtype), nan((C,), dtype), 0


def run_bn(c):
    """One BatchNorm case -> its outputs under the oracle's names (mode bn: ofa_batchnorm_fwd / _bwd; groups: ofa_batchnorm_fwd_apply
    behind the case's partial rows; sync: the four SyncBatchNorm entry points on rows A and B, their sums added on the device)."""
    x_all, na = c["x"], c["na"]
    rows_all, C = x_all.shape
    dtype, code = x_all.dtype, CODE[x_all.dtype]
    xa = x_all[:na].contiguous()
    y, mean, rstd = nan(xa.shape, dtype), nan((C,), F32), nan((C,), F32)
    rm, rv = c["rm0"].clone(), c["rv0"].clone()
    relu, eps, mom = int(c["relu"]), float(c["eps"]), float(c["mom"])
    out = dict(y=y, mean=mean, rstd=rstd)
    tot = None
    if c["mode"] == "bn":
        _call("ofa_batchnorm_fwd", xa, c["gamma"], c["beta"], c["res"], y, mean, rstd, rm, rv, ws_for(C), na, C, eps, mom, int(not c["train"]),
              relu, code)
    elif c["mode"] == "groups":
        _call("ofa_batchnorm_fwd_apply", xa, c["gamma"], c["beta"], c["res"], y, mean, rstd, rm, rv, c["partial"].contiguous(),
              c["partial"].shape[0], na, C, eps, mom, relu, code)
    else:
        xb = x_all[na:].contiguous()
        sa, sb = nan((2 * C + 1,), torch.float64), nan((2 * C + 1,), torch.float64)
        _call("ofa_batchnorm_fwd_stats", xa, sa, ws_for(C), na, C, code)
        _call("ofa_batchnorm_fwd_stats", xb, sb, ws_for(C), rows_all - na, C, code)
        tot = sa + sb
        assert float(tot[2 * C]) == rows_all
        _call("ofa_batchnorm_fwd_apply", xa, c["gamma"], c["beta"], c["res"], y, mean, rstd, rm, rv, tot, 0, na, C, eps, mom, relu, code)
    if c["train"]:
        out.update(running_mean=rm, running_var=rv)
    if not c["bwd"]:
        return out
    dya = c["dy"][:na].contiguous()
    dx = nan(xa.shape, dtype)
    dres = nan(xa.shape, dtype) if c["want_dres"] else None
    dgamma, dbeta, acc = _grads(c, C, dtype)
    gate_y = y if c["gate"] == "y" else None
    beta = c["beta"] if c["gate"] == "x" else None
    if c["mode"] == "bn":
        ws = ws_for(C)
        _call("ofa_batchnorm_bwd", dya, gate_y, xa, c["gamma"], mean, rstd, dx, dres, dgamma, dbeta, ws, na, C, int(c["train"]), relu, acc, beta, code)
        sums = ws[4 * 256 * C:4 * 256 * C + 2 * C].view(2, C).clone()
    else:
        assert c["gate"] != "y", "the other rank's y is not computed here"
        xb, dyb = x_all[na:].contiguous(), c["dy"][na:].contiguous()
        s_a, s_b = nan((2, C), F32), nan((2, C), F32)
        _call("ofa_batchnorm_bwd_stats", dya, None, xa, c["gamma"], mean, rstd, s_a, dgamma, dbeta, ws_for(C), na, C, relu, acc, beta, code)
        _call("ofa_batchnorm_bwd_stats", dyb, None, xb, c["gamma"], mean, rstd, s_b, nan((C,), dtype), nan((C,), dtype), ws_for(C), rows_all - na,
              C, relu, 0, beta, code)
        sums = s_a + s_b
        _call("ofa_batchnorm_bwd_dx", dya, None, xa, c["gamma"], mean, rstd, sums, dx, dres, na, tot[2 * C:], C, relu, beta, code)
    out.update(dx=dx, dgamma=dgamma, dbeta=dbeta, sums=sums)
    if c["want_dres"]:
        out["dres"] = dres
    return out
