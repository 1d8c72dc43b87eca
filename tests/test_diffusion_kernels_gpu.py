"""GPU: the three passes of csrc/diffusion.hip -- ofa_diffusion_q_sample, ofa_film_fwd / ofa_film_bwd, ofa_diffusion_loss -- per element
against the float64 restatement (tests/diffusion_oracle.py) on the same rounded inputs and the same fp32 schedule tables, in the three
dtypes.  Bounds are worked out from the arithmetic the header describes, not from what the kernels return:

  q-sample   x_t = fma(a, x0, s * noise): the product s * noise and the fma round in fp32 -> 2^-23 (|a x0| + |s noise|) covers both; the
             in-betweening mix fma(kw, x0, (1 - kw) x_t) adds a product and an fma rounding -> (1 - kw) times the first bound plus
             2^-23 (|kw x0| + |(1 - kw) x_t|); then half an ulp of the output dtype at the value (the one store rounding).
  FiLM       forward: fp32 (scale + 1) rounds, the fma rounds, the store rounds: REL (the stored dtype's half ulp times 2, as
             tests/test_tacotron_loss_gpu.py) of the two terms' magnitudes |(scale + 1) h| + |shift|; dh is one product: REL of itself.
             drows: an fp32 sum of n terms in any order is within n 2^-24 sum|terms| of the exact sum; n = the number of positions that
             take the row (T without row_of; the row's own positions, or every known position of the batch, with it); plus the store.
  loss       the project's bound for such sums, 1e-5 relative; dpred: REL / ABS as the tacotron test defines them."""
import pytest
import torch

from oracle import recipe
from tests import diffusion_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
REL = {torch.float32: 8 * 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
ABS = {torch.float32: 1e-37, torch.bfloat16: 1e-37, torch.float16: 2.0 ** -25}
SCALAR_REL = 1e-5
N_LEVELS = 1000
# (B, T, Dd, max_data_dim): one vector; 138 = 22 joints (rows neither 16-byte aligned nor whole vectors); 318 = 52 joints over several
# workgroups; Dd = max_data_dim (no padding column, aligned fp32 rows)
SHAPES = ((1, 1, 6, 8), (3, 5, 138, 512), (2, 70, 318, 512), (2, 5, 512, 512))
IDS = ["x".join(map(str, s)) for s in SHAPES]
_SCHEDULES = {}


def _schedule(prediction_type="sample"):
    from ofasys_amd.diffusion import NoiseSchedule
    if prediction_type not in _SCHEDULES:
        _SCHEDULES[prediction_type] = NoiseSchedule(num_train_timesteps=N_LEVELS, prediction_type=prediction_type)
    return _SCHEDULES[prediction_type]


def _levels(B):
    return torch.tensor([0, N_LEVELS - 1, N_LEVELS // 2 - 7][:B], dtype=torch.long)


def _lengths(B, T):
    return ([T, 1, max(1, T // 2)])[:B]


def _masks(B, T):
    return torch.arange(T).unsqueeze(0) >= torch.tensor(_lengths(B, T)).unsqueeze(1)


def _half_ulp(v, dtype):
    """Half the spacing of `dtype` at the float64 values v (subnormal range: the smallest spacing)."""
    bits, emin = {torch.float32: (24, -126), torch.bfloat16: (8, -126), torch.float16: (11, -14)}[dtype]
    e = torch.frexp(v.abs().clamp_min(1e-300))[1].double() - 1.0              # floor(log2 |v|)
    return torch.pow(2.0, e.clamp_min(emin) - bits)


# ------------------------------------------------------------------------------------------------------------------ q-sample
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_q_sample_against_the_float64_oracle(shape, dt):
    from ofasys_amd import ops
    dtype = DTYPES[dt]
    B, T, Dd, W = shape
    tag = f"df.qs.{B}.{T}.{Dd}"
    x0, noise, t = recipe.floats(tag + ".x0", (B, T, Dd)), recipe.floats(tag + ".n", (B, T, Dd)), _levels(B)
    masks = _masks(B, T)
    kw_values = torch.tensor([0.0, 0.25, 1.0])
    known_w = kw_values[(torch.arange(B * T) % 3)].reshape(B, T)
    sched = _schedule()
    tab = sched.on(DEV)
    sa, sb = tab.sqrt_acp.cpu().double(), tab.sqrt_1m_acp.cpu().double()
    a, s = sa[t].view(-1, 1, 1), sb[t].view(-1, 1, 1)
    for kw, m in ((None, None), (None, masks), (known_w, masks), (known_w, None)):
        got = ops.diffusion_q_sample(x0.to(DEV), noise.to(DEV), t.to(DEV), sched, W, dtype, known_w=kw.to(DEV) if kw is not None else None,
                                     masks=m.to(DEV) if m is not None else None)
        again = ops.diffusion_q_sample(x0.to(DEV), noise.to(DEV), t.to(DEV), sched, W, dtype, known_w=kw.to(DEV) if kw is not None else None,
                                       masks=m.to(DEV) if m is not None else None)
        torch.cuda.synchronize()
        assert got.dtype == dtype and got.shape == (B, T, W) and torch.equal(got, again)
        got = got.cpu()
        want = O.adaptor_input(x0, noise, t, sa, sb, W, kw, m)
        xt_terms = (a * x0.double()).abs() + (s * noise.double()).abs()
        bound = 2.0 ** -23 * xt_terms
        if kw is not None:
            k = kw.double().unsqueeze(-1)
            xt = O.add_noise(x0, noise, t, sa, sb)
            bound = (1.0 - k) * bound + 2.0 ** -23 * ((k * x0.double()).abs() + ((1.0 - k) * xt).abs())
        bound = torch.nn.functional.pad(bound, (0, W - Dd)) + _half_ulp(want, dtype)
        err = (got.double() - want).abs()
        assert bool((err <= bound).all()), (kw is not None, m is not None, float((err / bound).max()))
        assert not got[:, :, Dd:].any()                                         # the padding columns: exact zeros
        if m is not None:
            assert not got[m].any()                                             # padded frames: exact zeros
        if kw is not None:
            keep = (kw == 1.0) & (~m if m is not None else torch.ones_like(masks))
            assert torch.equal(got[..., :Dd][keep], x0.to(dtype)[keep])         # known frames: x0, rounded once
            free = (kw == 0.0) & (~m if m is not None else torch.ones_like(masks))
            plain = ops.diffusion_q_sample(x0.to(DEV), noise.to(DEV), t.to(DEV), sched, W, dtype).cpu()
            assert torch.equal(got[free], plain[free])                          # unknown frames: x_t itself


def test_q_sample_refusals():
    from ofasys_amd import ops
    from ofasys_amd.lib import OfaError
    sched = _schedule()
    x = torch.zeros(2, 3, 18, device=DEV)
    t = torch.zeros(2, dtype=torch.long, device=DEV)
    with pytest.raises(OfaError, match="data_dim 18 exceeds max_data_dim 16"):
        ops.diffusion_q_sample(x, x, t, sched, 16, torch.bfloat16)
    with pytest.raises(OfaError, match="must be one fp32"):
        ops.diffusion_q_sample(x.bfloat16(), x, t, sched, 32, torch.bfloat16)
    with pytest.raises(OfaError, match="noise levels must be int64"):
        ops.diffusion_q_sample(x, x, t.int(), sched, 32, torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------------ FiLM
def _film_case(B, T, D, dtype, integers=False):
    tag = f"df.film.{B}.{T}.{D}"
    if integers:
        gen = lambda k, shape: torch.round(recipe.floats(tag + k, shape, 1.5)).clamp(-3, 3)       # noqa: E731
    else:
        gen = lambda k, shape: recipe.floats(tag + k, shape, 0.75)                                  # noqa: E731
    h, dout, rows = gen(".h", (B, T, D)).to(dtype), gen(".g", (B, T, D)).to(dtype), gen(".rows", (B + 1, 2 * D)).to(dtype)
    own = torch.arange(B, dtype=torch.int32).unsqueeze(1).expand(B, T)
    row_of = torch.where((torch.arange(T) % 3 == 1).unsqueeze(0).expand(B, T), torch.full_like(own, B), own).contiguous()
    return h, dout, rows, row_of


def _film_reference(h, dout, rows, row_of):
    hd, rd = h.double().requires_grad_(True), rows.double().requires_grad_(True)
    out = O.film(hd, rd, row_of)
    out.backward(dout.double())
    return out.detach(), hd.grad, rd.grad


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("D", (8, 256, 768))
def test_film_forward_and_backward_against_the_float64_oracle(D, dt):
    from ofasys_amd import kernels as K
    dtype = DTYPES[dt]
    for B in (1, 3):
        for T in (1, 5, 70):
            h, dout, rows, row_of = _film_case(B, T, D, dtype)
            for ro in (None, row_of):
                r = rows if ro is not None else rows[:B].contiguous()
                want, wdh, wdrows = _film_reference(h, dout, r, ro)
                dev = [x.to(DEV) for x in (h, dout, r)]
                rod = ro.to(DEV) if ro is not None else None
                out = K.film_fwd(dev[0], dev[2], rod)
                dh, drows = K.film_bwd(dev[1], dev[0], dev[2], rod)
                dh2, drows2 = K.film_bwd(dev[1], dev[0], dev[2], rod)
                torch.cuda.synchronize()
                assert torch.equal(dh, dh2) and torch.equal(drows, drows2) and torch.equal(out, K.film_fwd(dev[0], dev[2], rod))
                out, dh, drows = out.cpu(), dh.cpu(), drows.cpu()
                assert out.dtype == dh.dtype == drows.dtype == dtype and drows.shape == r.shape
                idx = ro.long() if ro is not None else torch.arange(B).unsqueeze(1).expand(B, T)
                sc, sh = r.double()[idx][..., :D], r.double()[idx][..., D:]
                mag = ((sc + 1.0) * h.double()).abs() + sh.abs()
                assert bool(((out.double() - want).abs() <= REL[dtype] * mag + ABS[dtype]).all()), ("fwd", B, T, ro is not None)
                assert bool(((dh.double() - wdh).abs() <= REL[dtype] * wdh.abs() + ABS[dtype]).all()), ("dh", B, T, ro is not None)
                # drows: per row, n = the positions that take it; sum|terms| from the float64 terms
                terms = torch.cat(((dout.double() * h.double()).abs(), dout.double().abs()), dim=-1)           # [B, T, 2D]
                onehot = torch.nn.functional.one_hot(idx, r.shape[0]).double()                                  # [B, T, R]
                n = onehot.sum((0, 1))                                                                          # the count used, per row
                sum_abs = torch.einsum("btr,btc->rc", onehot, terms)
                bound = n.unsqueeze(1) * 2.0 ** -24 * sum_abs + REL[dtype] * wdrows.abs() + ABS[dtype]
                assert bool(((drows.double() - wdrows).abs() <= bound).all()), ("drows", B, T, ro is not None, n.tolist())
                if ro is not None and T == 1:
                    assert not drows[B].any()                                   # nobody takes the shared row: zeros, written


@pytest.mark.parametrize("dt", list(DTYPES))
def test_film_is_exact_on_small_integers(dt):
    """Integers in [-3, 3]: every product and every fp32 sum is exact, so each stored value is the float64 result rounded once."""
    from ofasys_amd import kernels as K
    dtype = DTYPES[dt]
    for B, T, D in ((3, 70, 256), (1, 5, 8)):
        h, dout, rows, row_of = _film_case(B, T, D, dtype, integers=True)
        for ro in (None, row_of):
            r = rows if ro is not None else rows[:B].contiguous()
            want, wdh, wdrows = _film_reference(h, dout, r, ro)
            rod = ro.to(DEV) if ro is not None else None
            out = K.film_fwd(h.to(DEV), r.to(DEV), rod)
            dh, drows = K.film_bwd(dout.to(DEV), h.to(DEV), r.to(DEV), rod)
            torch.cuda.synchronize()
            assert torch.equal(out.cpu(), want.to(dtype)) and torch.equal(dh.cpu(), wdh.to(dtype))
            assert torch.equal(drows.cpu(), wdrows.to(dtype))


@pytest.mark.parametrize("dt", ("fp32", "bf16"))
def test_film_through_the_embedding_with_two_sentences_on_one_level(dt):
    """ops.embedding + ops.film as the adaptor calls them: sentences 0 and 2 draw the same level, so their two gathered rows -- two
    rows of the kernel's drows -- meet in one row of the table's gradient (the embedding backward), next to the shared level-0 row."""
    from ofasys_amd import ops
    dtype = DTYPES[dt]
    B, T, D, levels = 3, 5, 256, 12
    h, dout, _, row_of = _film_case(B, T, D, dtype)
    table = recipe.floats("df.film.table", (levels, 2 * D), 0.5).to(dtype)
    ids = torch.tensor([6, 3, 6, 0])
    td, hd = table.double().requires_grad_(True), h.double().requires_grad_(True)
    O.film(hd, td[ids], row_of).backward(dout.double())
    tg, hg = table.to(DEV).requires_grad_(True), h.to(DEV).requires_grad_(True)
    out = ops.film(hg, ops.embedding(ids.to(DEV), tg), row_of.to(DEV))
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    assert bool(((hg.grad.cpu().double() - hd.grad).abs() <= REL[dtype] * hd.grad.abs() + ABS[dtype]).all())
    terms = torch.cat(((dout.double() * h.double()).abs(), dout.double().abs()), dim=-1).sum((0, 1))     # every position, an upper bound
    # B * T terms at most in fp32, each gathered row rounded to the dtype, two of them added and rounded again
    bound = B * T * 2.0 ** -24 * terms + 3 * REL[dtype] * terms + ABS[dtype]
    got = tg.grad.cpu().double()
    assert bool(((got - td.grad).abs() <= bound).all())
    touched = torch.zeros(levels, dtype=torch.bool)
    touched[ids] = True
    assert not got[~touched].any() and bool(got[6].abs().gt(0).any()) and bool(got[0].abs().gt(0).any())


def test_film_refusals():
    from ofasys_amd import kernels as K
    from ofasys_amd.lib import OfaError
    h = torch.zeros(2, 3, 12, device=DEV)
    with pytest.raises(OfaError, match="D=12 must be a positive multiple of 8"):
        K.film_fwd(h, torch.zeros(2, 24, device=DEV))
    h = torch.zeros(2, 3, 16, device=DEV)
    with pytest.raises(OfaError, match="R=2 rows for B=2 sentences"):
        K.film_fwd(h, torch.zeros(2, 32, device=DEV), torch.zeros(2, 3, dtype=torch.int32, device=DEV))
    with pytest.raises(OfaError, match="rows .* \\[R, 2D\\]"):
        K.film_fwd(h, torch.zeros(2, 16, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ loss
def _loss_case(shape, dtype):
    B, T, Dd, W = shape
    tag = f"df.loss.{B}.{T}.{Dd}"
    x0, noise = recipe.floats(tag + ".x0", (B, T, Dd)), recipe.floats(tag + ".n", (B, T, Dd))
    pred = recipe.floats(tag + ".pad", (B, T, W), 3.0)                          # (columns >= Dd hold values nobody may read)
    pred[..., :Dd] = x0 + recipe.floats(tag + ".d", (B, T, Dd), 0.5)
    pred = pred.to(dtype)
    x0[..., 0] = pred[..., 0].float()                                           # pred == target: the gradient there is exactly 0
    noise[..., 0] = pred[..., 0].float()
    return pred, x0, noise


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("prediction_type", ("sample", "epsilon"))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_loss_and_gradient_against_the_float64_oracle(shape, prediction_type, dt):
    from ofasys_amd import kernels as K
    dtype = DTYPES[dt]
    B, T, Dd, W = shape
    pred, x0, noise = _loss_case(shape, dtype)
    t, scale = _levels(B), 0.75
    sched = _schedule(prediction_type)
    w_dev = sched.on(DEV).w if prediction_type == "sample" else None
    w64 = sched.on(DEV).w.cpu().double()
    target = x0 if prediction_type == "sample" else noise
    for masks in (_masks(B, T), None):
        p64 = pred.double().requires_grad_(True)
        want = O.criterion(p64[..., :Dd], x0, noise, t, w64, prediction_type, masks, scale)
        want.backward()
        want, wgrad = float(want.detach()), p64.grad
        dev = dict(pred=pred.to(DEV), target=target.to(DEV), t=t.to(DEV), w=w_dev, scale=scale, masks=masks.to(DEV) if masks is not None else None)
        out, d = K.diffusion_loss(**dev, grad=True)
        out0, none = K.diffusion_loss(**dev)
        out2, d2 = K.diffusion_loss(**dev, grad=True)
        _, d128 = K.diffusion_loss(**dev, grad=True, seed=torch.full((), 128.0, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize()
        assert out.dtype == torch.float32 and out.shape == (1,) and none is None
        assert abs(float(out) - want) <= SCALAR_REL * abs(want), (float(out), want, masks is not None)
        assert torch.equal(out0, out) and torch.equal(out2, out) and torch.equal(d2, d)       # flag off: the same scalar; equal bits
        g, g128 = d.cpu(), d128.cpu()
        assert g.dtype == dtype and g.shape == (B, T, W)
        assert bool(((g.double() - wgrad).abs() <= REL[dtype] * wgrad.abs() + ABS[dtype]).all()), (masks is not None,)
        assert not g[..., Dd:].any() and not g128[..., Dd:].any()                # padding columns
        assert not g[..., 0].any()                                              # pred == target
        if masks is not None:
            assert not g[masks].any() and not g128[masks].any()                 # masked frames
            live = g[..., 1:Dd][~masks]
        else:
            live = g[..., 1:Dd]
        assert bool(live.abs().gt(0).all()) or dtype == torch.float16           # (fp16: the smallest gradients may round to 0)
        normal = g.double().abs() > (2.0 ** -14 if dtype == torch.float16 else 0.0)
        assert torch.equal(g128[normal].double(), 128 * g[normal].double())     # a seed of 128 scales every normal element exactly


@pytest.mark.parametrize("dt", ("fp32", "bf16"))
def test_loss_autograd_function_with_and_without_a_known_seed(dt):
    """ops.diffusion_loss: a seed told in advance makes the forward's one launch write the gradient; without one the backward runs the
    kernel at the scale it is given.  Both give the oracle's gradient; ops.diffusion_eval gives the same scalar."""
    from ofasys_amd import ops
    dtype, shape = DTYPES[dt], (3, 5, 138, 512)
    B, T, Dd, W = shape
    pred, x0, noise = _loss_case(shape, dtype)
    t, masks, sched = _levels(B), _masks(B, T), _schedule()
    p64 = pred.double().requires_grad_(True)
    want = O.criterion(p64[..., :Dd], x0, noise, t, sched.on(DEV).w.cpu().double(), "sample", masks, 1.0)
    want.backward()
    seed = torch.ones((), dtype=torch.float32, device=DEV)
    runs = []
    for known, scale in ((True, 1.0), (False, 1.0), (False, 64.0)):
        p = pred.to(DEV).requires_grad_(True)
        loss = ops.diffusion_loss(p, x0.to(DEV), t.to(DEV), sched, masks=masks.to(DEV), seed=seed if known else None)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        loss.backward(seed if known else torch.full((), scale, dtype=torch.float32, device=DEV))
        torch.cuda.synchronize()
        assert abs(float(loss) - float(want)) <= SCALAR_REL * float(want)
        assert bool(((p.grad.cpu().double() - scale * p64.grad).abs() <= REL[dtype] * scale * p64.grad.abs() + ABS[dtype]).all())
        runs.append(p.grad.clone())
    assert torch.equal(runs[0], runs[1])
    ev = ops.diffusion_eval(pred.to(DEV), x0.to(DEV), t.to(DEV), sched, masks=masks.to(DEV))
    assert abs(float(ev) - float(want)) <= SCALAR_REL * float(want)
