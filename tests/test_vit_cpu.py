"""CPU half of the image_vit tests: the oracle of tests/vit_oracle.py is sound (the clean emulation stays under CEILING, every mutation
exceeds it), its slab table is the library's, bad arguments come back as status codes, the adaptor's config / state-dict keys are the
golden's, the plain-torch restatement reproduces the golden's recorded outputs and gradients, and registering the adaptor changes no
existing model."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from ofasys_amd.adaptor.image_vit import ImageVitAdaptorConfig
from ofasys_amd.module import vit
from tests import vit_case as C
from tests import vit_oracle as O
from tests.golden_util import load_golden, rel_err


@pytest.fixture(scope="module")
def golden():
    return load_golden("vit")


# ------------------------------------------------------------------------------------------------------------------ the QuickGELU oracle
@pytest.fixture(scope="module")
def emulation_figures():
    """{(dtype, mutation or None): {output: worst excess over the table}}, computed once."""
    worst = {}
    for dtype in O.DTYPES3:
        for mut in (None,) + (O.MUTATIONS if dtype != O.F32 else ()):
            w = {}
            for case in O.CASES:
                h, dy = O.build(case, dtype)
                f = O.figures(O.qgelu_reference(h, dy), O.qgelu_emulate(h, dy, dtype, mut), dtype)
                for k, v in f.items():
                    w[k] = max(w.get(k, 0.0), v)
            worst[(dtype, mut)] = w
    return worst


@pytest.mark.parametrize("dtype", O.DTYPES3, ids=lambda d: O.NAMES[d])
def test_clean_emulation_stays_under_ceiling(emulation_figures, dtype):
    w = emulation_figures[(dtype, None)]
    print(O.NAMES[dtype], {k: (f"{v:.3e}" if dtype == O.F32 or k == "partial" else f"{v:.3f}") for k, v in w.items()})
    for name in O.OUTPUTS + ("partial",):
        assert w[name] <= O.limit(name, dtype, kernel=False), (name, w[name])


@pytest.mark.parametrize("mutation", O.MUTATIONS)
@pytest.mark.parametrize("dtype", (O.BF16, O.FP16), ids=lambda d: O.NAMES[d])
def test_every_mutation_exceeds_ceiling(emulation_figures, dtype, mutation):
    w = emulation_figures[(dtype, mutation)]
    print(O.NAMES[dtype], mutation, {k: f"{v:.3g}" for k, v in w.items()})
    assert max(w[n] for n in O.OUTPUTS) > O.CEILING, w


def test_saturated_rows_are_exact():
    """+30 / +80 come back exactly, +-0 as zero, -30 / -80 within the underflow floor of 0 (the emulation; the GPU test asks the kernel)."""
    for dtype in O.DTYPES3:
        case = next(c for c in O.CASES if c.regime == "sat" and c.m == 3 and c.rows == 3)
        h, dy = O.build(case, dtype)
        a = O.qgelu_emulate(h, dy, dtype)["a"]
        pos = h.float() > 0
        assert torch.equal(a[pos], h[pos]) and bool((a[h.float() == 0] == 0).all())
        assert float(a[h.float() < 0].float().abs().max()) <= (1e-20 if dtype != O.FP16 else O.floor_of(dtype))


def test_slab_table_is_the_librarys():
    from ofasys_amd.lib import lib
    cdll = lib().cdll
    for dtype in O.DTYPES3:
        for rows in sorted({c.rows for c in O.CASES} | {0, 32, 64, 65, 6272, 8192, 8193, 100000, 1 << 22}):
            for m in O.M:
                assert cdll.ofa_quick_gelu_bwd_slots(rows, m * O.NVEC[dtype], O.CODE[dtype]) == O.slots_of(rows), (rows, m)
    assert O.slots_of(O.ROWS_PER_BLOCK - 1) == 1 and O.slots_of(O.ROWS_PER_BLOCK + 1) == 2
    # the large cases are what they claim: one row past a full sweep of the forward's grid; slabs of more than 32 rows, the last ragged
    assert (O.SWEEP_ROWS - 1) * O.M[-1] >= O.FWD_GRID * O.FWD_BLOCK > (O.SWEEP_ROWS - 2) * O.M[-1]
    assert O.rows_per_block(O.SLAB_ROWS) == 36 and O.slots_of(O.SLAB_ROWS) == 228 and O.SLAB_ROWS % 36 != 0
    assert {(c.m, c.rows) for c in O.CASES} >= {(O.M[-1], O.SWEEP_ROWS), (O.M[0], O.SLAB_ROWS)}


def test_bad_arguments_return_status_codes():
    from ofasys_amd.lib import lib
    cdll = lib().cdll
    OK, INVALID, UNSUPPORTED = 0, 1, 2
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15                       # (host memory: every call below returns before any launch)
    fwd, bwd = cdll.ofa_quick_gelu_fwd, cdll.ofa_quick_gelu_bwd
    assert fwd(p, p, 0, 8, 1, None) == OK and bwd(p, p, p, None, 0, 8, 1, None) == OK        # rows == 0: nothing to do
    assert fwd(None, None, 0, 8, 1, None) == OK
    for dt, cols in ((1, 12), (2, 4), (0, 6), (1, 7)):
        assert fwd(p, p, 4, cols, dt, None) == UNSUPPORTED and bwd(p, p, p, None, 4, cols, dt, None) == UNSUPPORTED
        assert b"16-byte" in cdll.ofa_last_error()
    assert fwd(p, p, 4, 8, 7, None) == INVALID and bwd(p, p, p, None, 4, 8, -1, None) == INVALID
    assert fwd(p, p, -1, 8, 1, None) == INVALID and fwd(p, p, 4, 0, 1, None) == INVALID
    assert fwd(None, p, 4, 8, 1, None) == INVALID and bwd(p, None, p, None, 4, 8, 1, None) == INVALID
    assert fwd(p + 2, p, 4, 8, 1, None) == UNSUPPORTED and bwd(p, p, p, p + 4, 4, 8, 1, None) == UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------ config and keys
def test_config_fields_and_defaults_are_the_goldens(golden):
    want = [str(s) for s in golden["model.cfg_defaults"]]
    have = {}
    for f in dataclasses.fields(ImageVitAdaptorConfig):
        if not f.name.startswith("_"):
            v = f.default if f.default is not dataclasses.MISSING else None
            have[f.name] = v if isinstance(v, (int, float, bool, type(None))) else str(v)
    assert [f"{k}={v!r}" for k, v in have.items()] == want
    cfg = ImageVitAdaptorConfig()
    assert cfg.is_active is False and cfg.vit_type == "vit_base" and cfg.vit_drop_path_rate == 0.0 and cfg.image_bucket_size == 42


@pytest.fixture(scope="module")
def vit_model():
    from tests.model_util import build_model
    return build_model(C.MODEL_CASE)[0]


def test_state_dict_keys_and_shapes_are_the_goldens(golden, vit_model):
    state = vit_model.encoder.adaptor.image_vit.state_dict()
    assert [f"{k}|{tuple(v.shape)}" for k, v in state.items()] == [str(s) for s in golden["model.state_keys"]]
    assert "image_vit" not in dict(vit_model.decoder.adaptor.named_children())


def test_factories_have_the_reference_sizes():
    for fn, (res, p, width, layers, heads) in ((vit.vit_base, (224, 16, 768, 9, 12)), (vit.vit_large, (224, 14, 1024, 18, 16)),
                                               (vit.vit_large_336, (336, 14, 1024, 18, 16)), (vit.vit_huge, (224, 14, 1280, 24, 16))):
        with torch.device("meta"):
            m = fn()
        assert (m.input_resolution, m.patch_size, m.width, len(m.transformer.resblocks), m.transformer.resblocks[0].attn.num_heads) == \
            (res, p, width, layers, heads)
        assert m.positional_embedding.shape == ((res // p) ** 2 + 1, width) and m.conv1.bias is None
    with pytest.raises(NotImplementedError):
        vit.vit_base(0.1)


def test_pretrained_path_and_drop_path_are_refused():
    from tests.model_util import build_model
    for kv in ({"pretrained_ckpt_path": "somewhere.pt"}, {"vit_drop_path_rate": 0.1}):
        case = dict(C.MODEL_CASE, adaptor_overrides={"image_vit": dict(C.MODEL_CASE["adaptor_overrides"]["image_vit"], **kv)})
        with pytest.raises(NotImplementedError):
            build_model(case)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _grad_check(golden, tag, params, bound=1e-3):
    keys = [str(k) for k in golden[tag + ".gkeys"]]
    counts, norms, flat = golden[tag + ".gcount"], golden[tag + ".gnorm"], torch.from_numpy(golden[tag + ".gsample"])
    worst, o = 0.0, 0
    for k, n, want in zip(keys, counts, norms):
        g = params[k].grad
        e_norm = abs(float(g.double().norm()) - want) / want
        e_s = rel_err(C.sample(g), flat[o:o + n])
        o += int(n)
        worst = max(worst, e_norm, e_s)
        assert e_norm < bound and e_s < bound, (k, e_norm, e_s)
    return worst


@pytest.mark.parametrize("name", list(C.BACKBONE_CASES))
def test_restated_backbone_reproduces_the_golden(golden, name):
    (res, p, width, layers, heads), _ = C.BACKBONE_CASES[name]
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in vit.VisionTransformer(res, p, width, layers, heads).state_dict().items()}
    state = {k: torch.empty(s, dtype=torch.float64) for k, s in shapes.items()}
    C.fill_backbone_state(name, state)
    for v in state.values():
        v.requires_grad_(True)
    img, dout = C.backbone_inputs(name)
    y = O.vit_backbone(state, res, p, heads, img.double())
    (y * dout.double()).sum().backward()
    e = rel_err(y.detach(), torch.from_numpy(golden[f"bb.{name}.out"]))
    worst = _grad_check(golden, "bb." + name, state)
    print(name, "output", f"{e:.2e}", "gradients (norms and samples) worst", f"{worst:.2e}")
    assert e < 1e-3


def test_restated_adaptor_embed_reproduces_the_golden(golden, vit_model):
    from oracle.cases import make_value
    state = {k: v.detach().double() for k, v in vit_model.state_dict().items() if k.startswith(C.MODEL_PREFIX)}
    img = make_value(C.MODEL_CASE["slots"][0][2], 0)
    with torch.no_grad():
        y = O.vit_adaptor_embed(state, C.MODEL_PREFIX, 224, 16, 12, img.double())
    e = rel_err(y.reshape(-1)[::C.EMBED_STRIDE], torch.from_numpy(golden["model.embed"]))
    print("adaptor embed", f"{e:.2e}")
    assert e < 1e-3


# ------------------------------------------------------------------------------------------------------------------ nobody else changes
def test_inactive_adaptor_is_never_constructed():
    """What this shows: image_vit is registered but inactive by default, the model then has no such module, and building it never reaches
    the adaptor's constructor (replaced here by one that raises) -- so an inactive image_vit draws no random numbers.  Both builds are of
    the present code: that the initial bits equal those from before the adaptor existed (and from before ImageResnetAdaptor's shared
    code moved into ImageGridAdaptor) is pinned by tests/test_init_cpu.py against its recorded golden, not here."""
    from oracle.cases import CASES
    from ofasys_amd import Dictionary, GeneralistModel
    from ofasys_amd.adaptor import image_vit

    def make():
        d = Dictionary()
        for i in range(20):
            d.add_symbol(f"<text>_{i}")
        torch.manual_seed(3)
        m = GeneralistModel()
        m.cfg.arch = "tiny"
        m.__init__(m.cfg)
        for a in CASES["tiny_text"]["active"]:
            getattr(m.cfg.adaptor, a).is_active = True
        assert m.cfg.adaptor.image_vit.is_active is False
        m.initialize(d)
        return m.state_dict()

    a = make()
    orig = image_vit.ImageVitAdaptor.__init__
    image_vit.ImageVitAdaptor.__init__ = lambda *args, **kw: (_ for _ in ()).throw(AssertionError("constructed"))
    try:
        b = make()
    finally:
        image_vit.ImageVitAdaptor.__init__ = orig
    assert list(a) == list(b) and not any("image_vit" in k for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    np.testing.assert_equal(len(a), len(b))
