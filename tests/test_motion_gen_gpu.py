"""GPU: ofa_diffusion_sample_step per element against the float64 restatement (tests/motion_gen_oracle.py), and DiffusionGenerator end to
end on the tiny case of tests/diffusion_case.py.

Bounds.  The fp32 outputs (x_t, img) are held to 4x the largest error of the SAME restatement run in fp32 torch on the CPU against
float64 (the margin covers another summation order and a reciprocal against a division); both are measured per case and written with
the bound to profiles/motion_gen_parity.txt.  The denoiser input is held to one unit in the last place of the model dtype around the
float64 mix, rounded to that dtype, of the state the launch wrote (the state itself carries the bound above: a result that cancels to
1e-5 has an fp32-arithmetic error of many of ITS units in any implementation) -- and, against the all-float64 chain, to that unit plus
the state's bound."""
import os

import pytest
import torch

from tests import diffusion_case as C
from tests import motion_gen_oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, G = 4, 2.5
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def parity_file():
    yield
    if RECORD:
        with open(os.path.join(ROOT, "profiles", "motion_gen_parity.txt"), "w") as f:
            f.write("tests/test_motion_gen_gpu.py: largest |error| against float64 -- the kernel path, the fp32 restatement, the bound (4x the latter)\n")
            f.writelines(f"{k}: {v}\n" for k, v in sorted(RECORD.items()))


def _ulp(r, dtype):
    """One unit in the last place of r (a tensor of `dtype`), as float64."""
    bits = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}[dtype]
    return torch.ldexp(torch.ones_like(r, dtype=torch.float64), torch.frexp(r.double())[1] - 1 - bits)


def _rotations(gen, *shape):
    q, r = torch.linalg.qr(torch.randn(*shape, 3, 3, generator=gen, dtype=torch.float64))
    return (q * torch.sign(torch.diagonal(r, dim1=-2, dim2=-1)).unsqueeze(-2))[..., :2].transpose(-1, -2).reshape(*shape, 6)


def _frames(gen, T, Dd, sigma):
    """[B, T, Dd] float64: hip columns N(0, 1); per joint two columns of a random rotation plus N(0, sigma)."""
    joints = _rotations(gen, B, T, Dd // 6 - 1).reshape(B, T, Dd - 6)
    x = torch.cat((torch.randn(B, T, 6, generator=gen, dtype=torch.float64), joints), dim=-1)
    return x + sigma * torch.randn(B, T, Dd, generator=gen, dtype=torch.float64) * (torch.arange(Dd) >= 6)


def _inbetween(T, generic):
    """known_w [B, T] and the dense interp_w [B, T, T].  Collation form: rows whose first and last frames are unknown, row 1 with a gap
    over frames T - 3, T - 2 (across the tile border when T = tile + 1), a row with one known frame.  generic: any two frames per row."""
    from ofasys_amd.preprocessor.motion import interpolate_weight
    kw = torch.zeros(B, T)
    for b, known in enumerate(((2, T // 2, T - 2), (0, T - 4, T - 1), (T // 3,), (1, 2, 3, T - 3))):
        kw[b, list(known)] = 1.0
    if not generic:
        return kw, torch.stack([interpolate_weight(k) for k in kw])
    w = torch.zeros(B, T, T)
    for k in range(T):
        w[:, k, (k + 5) % T] += 0.3
        w[:, k, (3 * k + 1) % T] += 0.6
    return kw, w


@pytest.mark.parametrize("kind", ("ddim_mid", "ddim_last", "ddpm", "first"))
@pytest.mark.parametrize("mode", ("plain", "masks", "inbetween", "inbetween_generic", "guidance"))
@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=("bf16", "fp32"))
@pytest.mark.parametrize("T,Dd,W", ((13, 18, 24), (17, 138, 512)))
def test_step_kernel_against_float64(T, Dd, W, dtype, mode, kind):
    from ofasys_amd import kernels as K
    from ofasys_amd import ops
    from ofasys_amd.diffusion import NoiseSchedule
    assert T in (13, K.diffusion_step_frames() + 1)
    gen = torch.Generator().manual_seed(T * 1000 + Dd)
    ddim, first = kind != "ddpm", kind == "first"
    sched = NoiseSchedule(scheduler="DDIMScheduler" if ddim else "DDPMScheduler", num_train_timesteps=1000, num_inference_steps=50)
    plan = sched.sampling_plan()
    n = len(plan.timesteps)
    s = {"ddim_mid": 20, "ddim_last": n - 1, "ddpm": 7, "first": 0}[kind]
    level = O.levels(sched.acp, 1000, n, ddim)[s]
    guidance = G if mode == "guidance" else 0.0
    pred = _frames(gen, T, Dd, 0.2)
    if guidance:
        pred[1::2] = pred[0::2] + 0.1 * torch.randn(B // 2, T, Dd, generator=gen, dtype=torch.float64)
    pred = pred.to(dtype).double()                                         # what the kernel reads is the rounded prediction
    x_t = torch.randn(B, T, Dd, generator=gen)
    noise = None if ddim else torch.randn(n, B, T, Dd, generator=gen)
    masks = torch.arange(T)[None, :] >= torch.tensor([T, 1, T - 5, T // 2])[:, None] if mode == "masks" else None
    post = {}
    if mode.startswith("inbetween"):
        kw, interp_w = _inbetween(T, mode.endswith("generic"))
        post = dict(value_0=_frames(gen, T, Dd, 0.0).float(), known_w=kw, interp_w=interp_w)
    mix = {k: v for k, v in post.items() if k != "interp_w"}
    # the restatement, float64 and fp32
    want, err32 = {}, {}
    for dt in (torch.float64, torch.float32):
        if first:
            x_new, img = x_t.to(dt).clone(), None
            if guidance:
                x_new[1::2] = x_new[0::2]
        else:
            x_new, img = O.step(ddim, level, pred.to(dt), x_t.to(dt), None if ddim else noise[s], guidance=guidance, masks=masks, **post)
        got = {"x_t": x_new, "img": img}
        if dt == torch.float64:
            want = got
        else:
            err32 = {k: float((v.double() - want[k]).abs().max()) for k, v in got.items() if v is not None}
    # the kernel
    padded = torch.randn(B, T, W, generator=gen)                            # (what stands in the pad columns is never read)
    padded[..., :Dd] = pred
    st = {"x_t": x_t.clone(), "img": torch.zeros(B, T, Dd), "xin": torch.zeros(B, T, W, dtype=dtype), "level": torch.full((B,), -1),
          "counter": torch.tensor([0 if first else s, 0], dtype=torch.int32), "coef": torch.from_numpy(plan.coef).float(),
          "timesteps": torch.from_numpy(plan.timesteps.copy()), "masks": masks, "noise": noise}
    if post:
        st["nbr"], st["nbw"] = ops.diffusion_neighbours(post["interp_w"])
        st.update(mix)
    st = {k: v.to(DEV) for k, v in st.items() if v is not None}
    ops.diffusion_sample_step(None if first else padded.to(dtype).to(DEV), st, first=first, guidance_weight=guidance)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in st.items()}
    name = f"kernel T={T} Dd={Dd} {str(dtype)[6:]} {mode} {kind}"
    for k in err32:
        err = float((out[k].double() - want[k]).abs().max())
        RECORD[f"{name} {k}"] = f"kernel {err:.3e} fp32 restatement {err32[k]:.3e} bound {4 * err32[k]:.3e}"
        print(name, k, RECORD[f"{name} {k}"])
        assert err <= 4 * err32[k], (name, k, err, err32[k])
    # the denoiser input: rounded once from the written state; pad columns and padded frames untouched
    for state, slack in ((out["x_t"].double(), 0.0), (want["x_t"], 4 * err32["x_t"])):
        r = torch.nn.functional.pad(O.denoiser_input(state, masks=masks, **mix), (0, W - Dd)).to(dtype)
        assert bool(((out["xin"].double() - r.double()).abs() <= _ulp(r, dtype) + slack).all()), (name, slack)
    assert not out["xin"][..., Dd:].any() and (masks is None or not out["xin"][masks].any())
    assert out["level"].tolist() == [int(plan.timesteps[0 if first else min(s + 1, n - 1)])] * B
    assert out["counter"].tolist() == [0 if first else s + 1, 0]
    if guidance:
        assert torch.equal(out["x_t"][1::2], out["x_t"][0::2])


# ------------------------------------------------------------------------------------------------------------------ end to end
def _batch(d, inbetween):
    from ofasys_amd import ModalityType, Slot
    from ofasys_amd.preprocessor.motion import interpolate_weight
    masks = C.masks()
    value = {"value": torch.zeros(C.B, C.T, C.DD), "masks": masks}
    if inbetween:
        kw = torch.zeros(C.B, C.T)
        kw[:, 0] = 1.0
        kw[0, 5] = kw[0, 7] = 1.0
        gen = torch.Generator().manual_seed(5)
        value["value"] = _frames(gen, C.T, C.DD, 0.0)[:C.B].float().masked_fill(masks.unsqueeze(-1), 0.0)
        value["known_w"] = kw.masked_fill(masks, 0.0)
        value["interp_w"] = torch.stack([torch.nn.functional.pad(interpolate_weight(k[:n]), (0, C.T - n, 0, C.T - n))
                                         for k, n in zip(value["known_w"], C.LENGTHS)])
    value = {k: v.to(DEV) for k, v in value.items()}
    value["value_0"] = value["value"]
    return {"net_input": {"slots": [Slot(ModalityType.TEXT, True, C.source_tokens(len(d)).to(DEV)),
                                    Slot(ModalityType.MOTION, False, value, attributes=["adaptor=motion_6d"])]}}


def _python_loop(model, batch, sched, x_T, noise, dt):
    """The reference's loop over the same model calls, the step in `dt` arithmetic on the CPU."""
    from ofasys_amd import Slot
    slots = batch["net_input"]["slots"]
    v = slots[1].value
    ddim = sched.scheduler == "DDIMScheduler"
    lv = O.levels(sched.acp, sched.num_train_timesteps, sched.num_inference_steps, ddim)
    masks = v["masks"].cpu()
    post = dict(value_0=v["value_0"].cpu(), known_w=v["known_w"].cpu(), interp_w=v["interp_w"].cpu()) if "known_w" in v else {}
    mix = {k: t for k, t in post.items() if k != "interp_w"}
    with torch.no_grad():
        enc = model.encoder(slots[:1])
        x_t = x_T.to(dt)
        for i, level in enumerate(lv):
            xin = torch.nn.functional.pad(O.denoiser_input(x_t, masks=masks, **mix).float(), (0, 32 - C.DD)).to(DEV)
            value = {"value": xin, "masks": v["masks"], "noise_level": torch.full((C.B,), level[0], device=DEV), "data_dim": C.DD}
            if post:
                value["known_w"] = v["known_w"]
            pred, _ = model.decoder([Slot(slots[1].modality, False, value, attributes=slots[1].attributes)], encoder_out=enc,
                                    full_context_alignment=True)
            x_t, img = O.step(ddim, level, pred[..., :C.DD].cpu().to(dt), x_t, None if ddim else noise[i], masks=masks, **post)
    return img.double()


@pytest.mark.parametrize("inbetween", (False, True), ids=("plain", "inbetween"))
@pytest.mark.parametrize("scheduler", ("DDIMScheduler", "DDPMScheduler"))
def test_generator_graph_and_eager_agree_and_match_the_float64_loop(scheduler, inbetween):
    from ofasys_amd import DiffusionGenerator, MotionOutput
    from ofasys_amd.diffusion import NoiseSchedule
    from tests.model_util import build_model
    model, d = build_model(C.CASE, DEV, torch.float32)
    args = {"scheduler": scheduler, "num_train_timesteps": 20, "num_inference_steps": 4}
    gen = torch.Generator().manual_seed(11)
    x_T, noise = torch.randn(C.B, C.T, C.DD, generator=gen), torch.randn(4, C.B, C.T, C.DD, generator=gen)
    batch = _batch(d, inbetween)
    runs = {}
    for use_graph in (True, False):
        g = DiffusionGenerator(None, args, use_graph=use_graph)
        for _ in range(2):                                                  # (the second batch replays the captured step for all four steps)
            outs = g.generate(model, batch, x_T=x_T.to(DEV), noise=noise.to(DEV))
        assert g.captures == int(use_graph) and len(outs) == C.B and all(isinstance(o, MotionOutput) for o in outs)
        runs[use_graph] = torch.stack([o.feature for o in outs])
    assert torch.equal(runs[True], runs[False])
    sched = NoiseSchedule(**args)
    want = _python_loop(model, batch, sched, x_T, noise, torch.float64)
    gap = float((_python_loop(model, batch, sched, x_T, noise, torch.float32) - want).abs().max())
    err = float((runs[True].double() - want).abs().max())
    name = f"generator {scheduler} {'inbetween' if inbetween else 'plain'} img"
    RECORD[name] = f"generator {err:.3e} python loop with the fp32 step {gap:.3e} bound {4 * gap:.3e}"
    print(name, RECORD[name])
    assert gap > 0 and err <= 4 * gap
    assert not runs[True][C.masks()].any()                                  # padded frames are zeros


def test_task_inference_returns_orthonormal_rot6d_frames():
    from ofasys_amd import MotionOutput, Task, TaskConfig
    from ofasys_amd.preprocessor import to_device
    from tests.model_util import build_model
    model, d = build_model(C.CASE, DEV, torch.float32)
    tokens = C.source_tokens(len(d)).to(DEV)                                # (before initialize() adds the task's symbols to d)
    cfg = TaskConfig()
    cfg.diffuser_args = '{"num_train_timesteps": 20, "num_inference_steps": 4}'
    cfg.dataset.shuffle = False
    task = Task(cfg, name="t2m", instruction="[TEXT:text] -> [MOTION:motion,preprocess=motion_6d,adaptor=motion_6d,min_length=1]",
                micro_batch_size=C.B)
    task.initialize(d)
    task.add_dataset([{"text": f"motion {i}", "motion": torch.zeros(C.T, C.DD).numpy()} for i in range(C.B)], "valid")
    batch = to_device(task.get_sample("valid"), DEV)
    [s for s in batch["net_input"]["slots"] if s.is_src][0].value = tokens
    outs = task.inference(model, batch)
    assert len(outs) == C.B and all(isinstance(o, MotionOutput) and tuple(o.feature.shape) == (C.T, C.DD) for o in outs)
    j = torch.stack([o.feature for o in outs])[..., 6:].reshape(C.B, C.T, -1, 2, 3).double()
    gram = j @ j.transpose(-1, -2)
    assert float((gram - torch.eye(2, dtype=torch.float64)).abs().max()) <= 1e-5
