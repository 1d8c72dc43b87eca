"""GPU: ofa_tacotron2_loss (csrc/tacotron_loss.hip) against the float64 restatement of the reference's compute_loss
(tests/tts_oracle.py) -- the four scalars and the three gradients, both reductions, two positive weights, the three dtypes."""
import pytest
import torch

from oracle import recipe
from tests import tts_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# relative half-ulp of a stored gradient (the kernel computes in fp32 and rounds once) with a factor 2 of slack; fp32: a few fp32 roundings
REL = {torch.float32: 8 * 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ABS = {torch.float32: 1e-37, torch.bfloat16: 1e-37, torch.float16: 2.0 ** -25}       # fp16: half the subnormal spacing 2^-24
SCALAR_REL = 1e-5       # the scalars are fp32 sums of exact inputs: per-thread fp32 adds of a few elements, the rest in fp64, one rounding
# (B, T, F): a vectorised shape with one workgroup, one with 3 workgroups (51 frames each), and F = 6 (one element per access)
SHAPES = {(3, 11, 80): ([11, 7, 1],), (2, 70, 160): ([70, 1], [33, 70]), (2, 5, 6): ([5, 1], [3, 5])}


def _case(shape, lengths, dtype):
    B, T, F = shape
    tag = f"tl.{B}.{T}.{F}"
    tgt = recipe.floats(tag + ".tgt", shape).to(dtype)
    feat = (tgt.float() + recipe.floats(tag + ".feat", shape, 0.5)).to(dtype)
    post = (tgt.float() + recipe.floats(tag + ".post", shape, 0.25)).to(dtype)
    feat[:, :, 0] = tgt[:, :, 0]                                               # feat == tgt: the L1 term's gradient there is 0
    post[:, :, 1] = tgt[:, :, 1]
    eos = recipe.floats(tag + ".eos", (B, T, 1), 2.0)
    eos[0, 0, 0], eos[1, 0, 0] = 40.0, -40.0                                   # the stable form: log1p(exp(-40)), no overflow of exp(40)
    eos[0, lengths[0] - 1, 0] = -40.0                                          # ... also on a positive (last-frame) target
    return feat, post, eos.to(dtype), tgt, torch.tensor(lengths, dtype=torch.long)


def _reference(feat, post, eos, tgt, lengths, pw, reduction):
    f, p, e = (t.double().requires_grad_(True) for t in (feat, post, eos))
    out = O.tacotron2_loss(f, p, e, tgt.double(), lengths, pw, reduction)
    out[0].backward()
    return torch.stack([o.detach() for o in out]), (f.grad, p.grad, e.grad)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("pw", (1.0, 5.5))
@pytest.mark.parametrize("reduction", ("mean", "sum"))
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_loss_and_gradients_against_the_float64_oracle(shape, reduction, pw, dt):
    from ofasys_amd import kernels as K
    dtype = DTYPES[dt]
    B, T, F = shape
    for lengths in SHAPES[shape]:
        feat, post, eos, tgt, ln = _case(shape, lengths, dtype)
        want, wgrads = _reference(feat, post, eos, tgt, ln, pw, reduction)
        dev = [t.to(DEV) for t in (feat, post, tgt, eos, ln)]
        out, d = K.tacotron2_loss(*dev, pw, reduction, grad=True)
        out0, none = K.tacotron2_loss(*dev, pw, reduction)
        out2, d2 = K.tacotron2_loss(*dev, pw, reduction, grad=True)
        seed = torch.full((), 128.0, dtype=torch.float32, device=DEV)
        _, d128 = K.tacotron2_loss(*dev, pw, reduction, seed=seed, grad=True)
        torch.cuda.synchronize()
        # the four scalars; the flag-off form gives the same ones; two launches give equal bits
        assert out.dtype == torch.float32 and out.shape == (4,)
        assert bool(((out.double().cpu() - want).abs() <= SCALAR_REL * want.abs()).all()), (out.tolist(), want.tolist())
        assert none is None and torch.equal(out0, out) and torch.equal(out2, out)
        mask = (torch.arange(T)[None, :] < ln[:, None])
        for name, g, g2, g128, w in zip(("dfeat", "dpost", "deos"), d, d2, d128, wgrads):
            g, g128 = g.cpu(), g128.cpu()
            assert g.dtype == dtype and g.shape == w.shape and torch.equal(g2.cpu(), g)
            assert bool(((g.double() - w).abs() <= REL[dtype] * w.abs() + ABS[dtype]).all()), (name, lengths)
            assert not g[~mask].any() and not g128[~mask].any()                # padded frames: exact zeros
            assert bool(((g128.double() - 128 * w).abs() <= REL[dtype] * 128 * w.abs() + ABS[dtype]).all()), (name, lengths)
            # a seed of 128 scales the gradients exactly -- wherever the format scales: an fp16 value at or below the smallest normal
            # 2^-14 was rounded on the subnormal grid 2^-24, 128 times it on a finer one (a value rounded UP to 2^-14 included)
            normal = g.double().abs() > (2.0 ** -14 if dtype == torch.float16 else 0.0)
            assert torch.equal(g128[normal].double(), 128 * g[normal].double()), name
        # feat == tgt (post == tgt) elements: sign(0) = 0 and 2 d = 0 -> exactly 0
        assert not d[0].cpu()[:, :, 0].any() and not d[1].cpu()[:, :, 1].any()
        assert bool(d[0].cpu()[:, :, 2][mask].abs().gt(0).any())


@pytest.mark.parametrize("dt", ("fp32", "bf16"))
def test_autograd_function_with_and_without_a_known_seed(dt):
    """ops.tacotron2_loss: a seed told in advance makes the forward's one launch write the gradients and the backward hand them out;
    without one (loss scaling) the backward runs the kernel at the scale it is given.  Both give the oracle's gradients; the
    validation form gives the same scalars."""
    from ofasys_amd import ops
    dtype, shape, lengths = DTYPES[dt], (3, 11, 80), [11, 7, 1]
    feat, post, eos, tgt, ln = _case(shape, lengths, dtype)
    want, wgrads = _reference(feat, post, eos, tgt, ln, 5.5, "mean")
    seed = torch.ones((), dtype=torch.float32, device=DEV)
    runs = []
    for known, scale in ((True, 1.0), (False, 1.0), (False, 64.0)):
        f, p, e = (t.to(DEV).requires_grad_(True) for t in (feat, post, eos))
        loss, terms = ops.tacotron2_loss(f, p, e, tgt.to(DEV), ln.to(DEV), 5.5, "mean", seed=seed if known else None)
        assert loss.dim() == 0 and loss.dtype == torch.float32 and terms.shape == (3,) and not terms.requires_grad
        loss.backward(seed if known else torch.full((), scale, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize()
        assert abs(float(loss) - float(want[0])) <= SCALAR_REL * float(want[0])
        assert bool(((terms.double().cpu() - want[1:]).abs() <= SCALAR_REL * want[1:].abs()).all())
        for g, w in zip((f.grad, p.grad, e.grad), wgrads):
            assert g.shape == w.shape
            assert bool(((g.double().cpu() - scale * w).abs() <= REL[dtype] * scale * w.abs() + ABS[dtype]).all())
        runs.append([f.grad.clone(), p.grad.clone(), e.grad.clone()])
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))            # the precomputed gradient is the recomputed one
    ev = ops.tacotron2_eval(feat.to(DEV), post.to(DEV), eos.to(DEV), tgt.to(DEV), ln.to(DEV), 5.5, "mean")
    assert bool(((ev.double().cpu() - want).abs() <= SCALAR_REL * want.abs()).all())
