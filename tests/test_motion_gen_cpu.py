"""CPU half of the motion-generation tests: the sampling plan against the two-stage restatement (tests/motion_gen_oracle.py), the user
surface (Task.generator for a MOTION target) and the refusals of ofa_diffusion_sample_step that fire before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from ofasys_amd.diffusion import NoiseSchedule
from tests import motion_gen_oracle as O


@pytest.mark.parametrize("N,n", ((1000, 50), (20, 20), (10, 3)))
@pytest.mark.parametrize("scheduler,extra", (("DDIMScheduler", {}), ("DDPMScheduler", {}), ("DDIMScheduler", {"steps_offset": 1}),
                                             ("DDIMScheduler", {"set_alpha_to_one": False})))
def test_sampling_plan_is_the_two_stage_step(N, n, scheduler, extra):
    """The coefficients are what the restatement's step does to the unit inputs (it is linear), to 1e-12 of the row's largest."""
    s = NoiseSchedule(scheduler=scheduler, num_train_timesteps=N, num_inference_steps=n, **extra)
    if extra.get("steps_offset") and (n - 1) * (N // n) + 1 >= N:           # (20, 20): the offset leaves the table
        with pytest.raises(ValueError, match="outside the 20 training levels"):
            s.sampling_plan()
        return
    plan, ddim = s.sampling_plan(), scheduler == "DDIMScheduler"
    lv = O.levels(s.acp, N, n, ddim, extra.get("steps_offset", 0), extra.get("set_alpha_to_one", True))
    assert plan.timesteps.dtype == np.int64 and plan.timesteps.tolist() == [t for t, _, _ in lv] and plan.coef.shape == (n, 3)
    one, zero = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    for row, level in zip(plan.coef, lv):
        want = [float(O.scheduler_step(ddim, *unit, *level)) for unit in ((one, zero, zero), (zero, one, zero), (zero, zero, one))]
        assert max(abs(a - b) for a, b in zip(row, want)) <= 1e-12 * max(abs(w) for w in want), (level, row, want)
    if ddim and "set_alpha_to_one" not in extra:
        assert plan.coef[-1].tolist() == [1.0, 0.0, 0.0]
    if not ddim:
        assert plan.timesteps[-1] == 0 and plan.coef[-1, 2] == 0.0 and (plan.coef[:-1, 2] > 0).all()
    dev = s.sampling_on("cpu")
    assert dev.coef.dtype == torch.float32 and torch.equal(dev.coef, torch.from_numpy(plan.coef.astype(np.float32))) and dev is s.sampling_on("cpu")


def test_what_cannot_sample_raises():
    with pytest.raises(ValueError, match=r"num_inference_steps=11 must be in \[1, num_train_timesteps=10\]"):
        NoiseSchedule(num_train_timesteps=10, num_inference_steps=11).sampling_plan()
    with pytest.raises(ValueError, match="timestep 20 .steps_offset=1. is outside the 20 training levels"):
        NoiseSchedule(num_train_timesteps=20, num_inference_steps=20, steps_offset=1).sampling_plan()
    with pytest.raises(NotImplementedError, match="module/diffusion.py:140-143"):
        NoiseSchedule(prediction_type="epsilon").sampling_plan()
    assert NoiseSchedule(prediction_type="epsilon", num_inference_steps=5000).structure() == ("diffusion", "epsilon", 1000)    # training is as it was


def test_task_generator_for_a_motion_target_is_the_diffusion_generator(tmp_path):
    from ofasys_amd import Dictionary, DiffusionGenerator, MotionOutput, Task
    t = Task(name="t2m", instruction="[TEXT:text] -> [MOTION:motion,preprocess=motion_6d,adaptor=motion_6d]")
    t.initialize(Dictionary())
    t.cfg.evaluation.generator_args = '{"beam": 5, "max_len_b": 32, "guidance_weight": 2.5, "use_graph": false}'
    gen = t.generator
    assert isinstance(gen, DiffusionGenerator) and gen is t.generator and gen.diffusion is t.noise_schedule
    assert (gen.guidance_weight, gen.use_graph, gen.diffusion.num_inference_steps, gen.diffusion.clip_sample) == (2.5, False, 50, False)
    out = MotionOutput(feature=torch.ones(3, 18))
    out.save_features(str(tmp_path / "m"))
    assert np.load(tmp_path / "m.npz", allow_pickle=True)["feature"].shape == (3, 18)
    for save in (out.save_as_bvh, out.save_as_gif):
        with pytest.raises(NotImplementedError, match="needs the BVH header"):
            save("x")
    with pytest.raises(ValueError, match="a row with 3 non-zeros"):
        from ofasys_amd import ops
        ops.diffusion_neighbours(torch.ones(1, 3, 3))


@pytest.mark.parametrize("change,dtype,match", ((dict(B=3, guidance=2.5), 0, "B=3 is odd"), (dict(W=17), 0, "W=17 columns cannot hold Dd=18"),
                                                (dict(Dd=20, W=24), 1, "Dd = 6 \\+ 6 \\* joints"), ({}, 7, "bad dtype 7"),
                                                (dict(value_0=4096), 2, "in-betweening takes value_0, known_w and both")))
def test_step_entry_point_refuses_bad_arguments_before_any_launch(change, dtype, match):
    from ofasys_amd import kernels as K
    from ofasys_amd import lib as L
    assert "ofa_diffusion_sample_step" in L.parse_header() and K.diffusion_step_frames() == 16
    a = K._DiffusionStepArgs(pred=4096, x_t=4096, coef=4096, timesteps=4096, counter=4096, img=4096, xin=4096, level=4096, B=4, T=5, Dd=18,
                             W=24, n_steps=3)
    for k, v in change.items():
        setattr(a, k, v)
    with pytest.raises(L.OfaError, match=match):
        L.lib().call("ofa_diffusion_sample_step", ctypes.addressof(a), dtype, None)
