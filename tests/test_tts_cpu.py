"""CPU half of the text-to-speech tests: the plain-torch oracle (tests/tts_oracle.py) against tests/golden/tts.npz (the reference's own
run, tools/gen_tts_golden.py), the criterion route of a "target_lengths" micro-batch with its refusals, the target-side collation
against the reference's, and the C ABI of the new kernels (declared, exported, refusing bad arguments before any launch)."""
import ctypes
import itertools

import pytest
import torch

from oracle import recipe
from ofasys_amd import criterion
from tests import tts_case as C
from tests import tts_oracle as O
from tests.golden_util import load_golden, rel_err

FP32_BOUND = 1e-3
X = torch.zeros(1)


@pytest.fixture(scope="module")
def golden():
    return load_golden("tts")


def adaptor_state(golden, dtype=torch.float32):
    """The decoder-side adaptor's float entries from the shared recipe, under the model's keys."""
    state = {}
    for item in golden["state_keys"]:
        key, shape = str(item).split("|")
        shape = tuple(int(v) for v in shape.strip("()").split(",") if v.strip())
        if key.split(".")[-1] in ("audio_rp_bucket", "num_batches_tracked"):
            continue
        state[C.PREFIX + key] = recipe.value_for(C.PREFIX + key, shape).to(dtype)
    return state


# ------------------------------------------------------------------------------------------------------------------ oracle vs golden
def test_oracle_matches_the_golden(golden):
    """The restatement of the prenet, the output head with its postnet (train-mode BatchNorm over the padded frames) and the criterion
    against the reference's recorded run: the project's fp32 contract, 1e-3 relative (measured: profiles/tts_parity_measured.txt)."""
    state = adaptor_state(golden)
    g = {k: torch.from_numpy(golden[k]) for k in ("prev_outputs", "target", "hidden", "embed", "post", "feature_out", "eos_out")}
    lengths = torch.from_numpy(golden["target_lengths"])
    figs = {"embed": rel_err(O.prenet(state, C.PREFIX, g["prev_outputs"]), g["embed"])}
    post, feat, eos = O.head(state, C.PREFIX, g["hidden"], training=True)
    figs.update(post=rel_err(post, g["post"]), feature_out=rel_err(feat, g["feature_out"]), eos_out=rel_err(eos, g["eos_out"]))
    for reduction in ("mean", "sum"):
        got = torch.stack(O.tacotron2_loss(g["feature_out"].double(), g["post"].double(), g["eos_out"].double(), g["target"].double(),
                                           lengths, C.BCE_POS_WEIGHT, reduction))
        figs["loss_" + reduction] = rel_err(got, torch.from_numpy(golden["loss_" + reduction]))
    print({k: f"{v:.3e}" for k, v in figs.items()})
    assert all(v < FP32_BOUND for v in figs.values()), figs


def test_the_oracle_unfold_is_the_convolution(golden):
    """unfold1d (F.pad and index) times the (k, c)-ordered weight equals F.conv1d: the layout the kernels are tested against."""
    B, T, Cin, Cout, k = 2, 5, 6, 4, 3
    x, w = recipe.floats("tts.unfold.x", (B, T, Cin)).double(), recipe.floats("tts.unfold.w", (Cout, Cin, k)).double()
    col = O.unfold1d(x.reshape(B * T, Cin), B, T, Cin, k)
    assert col.shape == (B * T, 24) and torch.equal(col[:, k * Cin:], torch.zeros(B * T, 24 - k * Cin, dtype=col.dtype))
    y = col[:, :k * Cin] @ w.permute(0, 2, 1).reshape(Cout, k * Cin).t()
    want = torch.nn.functional.conv1d(x.transpose(1, 2), w, padding=1).transpose(1, 2).reshape(B * T, Cout)
    assert rel_err(y, want) < 1e-12


def test_the_adaptor_keeps_the_reference_state_dict(golden):
    from tests.model_util import build_model
    model, _ = build_model(C.CASE)
    ad = model.decoder.adaptor.name2adaptor["audio_fbank"]
    have = [f"{k}|{tuple(v.shape)}" for k, v in ad.state_dict().items()]
    assert have == [str(s) for s in golden["state_keys"]]
    assert callable(getattr(type(ad.prenet[0]), "forward")) and "residual" in type(ad.postnet).forward.__code__.co_varnames


# ------------------------------------------------------------------------------------------------------------------ the route
SETTINGS = [criterion.Settings(pad=1, eos=2, label_smoothing=ls, constraint_range=cr, drop_worst_ratio=dw, edge_head=head)
            for head, ls, cr, dw in itertools.product((False, True), (0.0, 0.1), (None, (4, 100)), (0.0, 0.25))]
TTS = {"target_lengths": X}
REFUSALS = [
    ("reward", dict(TTS, reward=X), "cannot carry reward"),
    ("nodes", dict(TTS, constraint_nodes=X, constraint_trie={"N": 1}), "cannot carry constraint_nodes"),
    ("masks", dict(TTS, constraint_masks=X), "cannot carry constraint_masks"),
    ("encoder_target", dict(TTS, encoder_target=X, ctc_range="8,40"), "cannot carry encoder_target"),
    ("pack", dict(TTS, pack=object()), "cannot carry a pack plan"),
    ("guided attention", dict(TTS, use_guided_attention_loss=True), "use_guided_attention_loss"),
    ("its own ctc", dict(TTS, ctc_weight=0.5), "ctc_weight > 0"),
]


def _route(extra, cfg, training):
    return criterion.route(dict({"slots": [], "target": X}, **extra), cfg, training)


def test_target_lengths_route_to_tacotron2_and_routes_is_unchanged():
    assert criterion.ROUTES == ("speech_to_text", "trie_head", "trie_nodes", "scst", "label_smoothed", "plain")
    assert criterion.EXTRA_ROUTES == ("tacotron2",) and not set(criterion.EXTRA_ROUTES) & set(criterion.ROUTES)
    for cfg in SETTINGS:
        for training in (True, False):
            assert _route(TTS, cfg, training) == "tacotron2"
            assert _route(dict(TTS, bce_pos_weight=5.5, sentence_avg=True, use_guided_attention_loss=False, ctc_weight=0.0, task="tts"),
                          cfg, training) == "tacotron2"


@pytest.mark.parametrize("name,extra,fragment", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_fires_in_route_with_its_message(name, extra, fragment):
    for cfg in SETTINGS[::3]:
        for training in (True, False):
            with pytest.raises(NotImplementedError, match=fragment):
                _route(extra, cfg, training)


def test_an_absent_key_and_a_key_set_to_none_route_alike():
    base = criterion.Settings(pad=1, eos=2)
    for extra in ({}, {"constraint_masks": X}, {"reward": X}, {"encoder_target": X, "ctc_range": "8,40"}, {"pack": object()}):
        for cfg in (base, base._replace(label_smoothing=0.1)):
            assert _route(extra, cfg, True) == _route(dict(extra, target_lengths=None), cfg, True) != "tacotron2"
    for k in ("reward", "constraint_nodes", "constraint_masks", "encoder_target", "pack", "use_guided_attention_loss", "ctc_weight"):
        assert _route(dict(TTS, **{k: None}), base, True) == "tacotron2"


# ------------------------------------------------------------------------------------------------------------------ collation
def _collated(attrs=None):
    from ofasys_amd import ModalityType, Slot
    from ofasys_amd.preprocessor import Dictionary, FbankPreprocess
    from ofasys_amd.preprocessor.collate import PreprocessConfig
    pre = FbankPreprocess(Dictionary(), PreprocessConfig(), ModalityType.AUDIO)
    slots = [pre.map(Slot(ModalityType.AUDIO, False, {"fbank": f, "fbank_lengths": f.shape[0]}, attributes=attrs)) for f in C.frames()]
    return pre.collate(slots)


def test_target_collation_equals_the_reference_bit_for_bit(golden):
    out = _collated()
    inp, tgt, extra = out.net_input_slot.value, out.net_target_slot.value, out.sample_extra
    assert torch.equal(inp["fbank"], torch.from_numpy(golden["prev_outputs"]))
    assert torch.equal(extra["target"], torch.from_numpy(golden["target"])) and torch.equal(tgt["fbank"], extra["target"])
    lengths = torch.from_numpy(golden["target_lengths"])
    assert extra["target_lengths"].dtype == torch.int64
    assert torch.equal(extra["target_lengths"], lengths) and torch.equal(inp["fbank_lengths"], lengths)
    assert extra["ntokens"] == int(golden["ntokens"][0]) == sum(C.FRAME_LENGTHS)
    assert not out.net_input_slot.is_src and torch.equal(inp["fbank"][:, 0], torch.zeros(C.B, C.F))


def test_pack_frames_equals_the_reference(golden):
    from ofasys_amd.preprocessor import pack_frames
    f0 = C.frames()[0]
    assert torch.equal(pack_frames(f0, C.PACK_N), torch.from_numpy(golden["packed0"]))
    assert pack_frames(f0, 1) is f0 and pack_frames(f0, 3).shape == (3, 3 * C.F)
    out = _collated(["n_frames_per_step=2"])
    assert out.sample_extra["target"].shape == (C.B, 5, 2 * C.F) and out.sample_extra["target_lengths"].tolist() == [5, 3, 0]


def test_source_side_and_tensor_values_collate_as_before():
    from ofasys_amd import ModalityType, Slot
    from ofasys_amd.preprocessor import Dictionary, FbankPreprocess, TensorPreprocess
    from ofasys_amd.preprocessor.collate import PreprocessConfig
    vals = [torch.full((4, 3), float(i)) for i in range(2)]
    for is_src in (True,):
        outs = [cls(Dictionary(), PreprocessConfig(), ModalityType.AUDIO).collate(
            [Slot(ModalityType.AUDIO, is_src, v.clone()) for v in vals]) for cls in (FbankPreprocess, TensorPreprocess)]
        assert torch.equal(outs[0].net_input_slot.value, outs[1].net_input_slot.value) and outs[0].net_target_slot is None


def test_a_task_collates_a_text_to_speech_sample():
    from ofasys_amd import Dictionary
    from ofasys_amd.task import Task
    task = Task(instruction="[TEXT:src] -> [AUDIO:fbank]", name="tts")
    task.cfg.criterion.name = "ofa_tacotron2"
    task.initialize(Dictionary())
    rows = [{"src": "hello world", "fbank": {"fbank": f, "fbank_lengths": f.shape[0]}} for f in C.frames()]
    s = task.collate(rows)
    assert s["target"].shape == (C.B, 11, C.F) and s["target_lengths"].tolist() == C.FRAME_LENGTHS and s["ntokens"] == 19
    tgt_in = [sl for sl in s["net_input"]["slots"] if not sl.is_src]
    assert len(tgt_in) == 1 and torch.equal(tgt_in[0].value["fbank"][:, 1:], s["target"][:, :-1])
    assert task.cfg.criterion.bce_pos_weight == 1.0 and task.cfg.criterion.use_guided_attention_loss is False


# ------------------------------------------------------------------------------------------------------------------ header, library, arguments
NEW = {"ofa_unfold1d": 9, "ofa_fold1d": 9, "ofa_tanh_dropout_fwd": 9, "ofa_tanh_dropout_bwd": 10, "ofa_tacotron2_loss": 20,
       "ofa_tacotron2_loss_blocks": 2}


def test_header_declares_and_library_exports_the_entry_points():
    from ofasys_amd.lib import lib, parse_header
    protos = parse_header()
    for name, nargs in NEW.items():
        assert name in protos and len(protos[name][1]) == nargs, name
    h = lib()
    for name in NEW:
        assert getattr(h.cdll, name)
    assert h.cdll.ofa_tacotron2_loss_blocks(19, 80) == 1 and h.cdll.ofa_tacotron2_loss_blocks(25600, 80) == 251
    assert h.cdll.ofa_tacotron2_loss_blocks(0, 80) == 0 and h.cdll.ofa_tacotron2_loss_blocks(3, 100000) == 3


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Status codes, no launch: every pointer here is a made-up address nothing may dereference (there is no device in this test)."""
    from ofasys_amd.lib import BF16, F16, F32, lib
    h = lib().cdll
    p = ctypes.c_void_p(4096)
    INVALID, UNSUPPORTED = 1, 2

    def loss(**kw):
        a = dict(feat=p, post=p, tgt=p, eos=p, lengths=p, B=2, T=5, F=80, pw=1.0, red=0, seed=None, partial=p, out=p, dfeat=None,
                 dpost=None, deos=None, grad=0, dt=BF16, tdt=BF16, st=None)
        a.update(kw)
        return h.ofa_tacotron2_loss(*a.values())

    for kw, code in ((dict(F=0), INVALID), (dict(F=-3), INVALID), (dict(red=2), INVALID), (dict(red=-1), INVALID),
                     (dict(tdt=F32), UNSUPPORTED), (dict(dt=F16, tdt=BF16), UNSUPPORTED), (dict(dt=7, tdt=7), INVALID),
                     (dict(B=0), INVALID), (dict(feat=None), INVALID), (dict(lengths=None), INVALID), (dict(out=None), INVALID),
                     (dict(grad=1), INVALID), (dict(grad=1, dfeat=p, dpost=p), INVALID)):
        assert loss(**kw) == code, kw
        assert b"tacotron2_loss" in h.ofa_last_error()

    for fn in (h.ofa_unfold1d, h.ofa_fold1d):
        assert fn(p, p, 0, 5, 8, 3, 24, BF16, None) == 0                                       # B == 0: nothing
        for args, code in (((p, p, 2, 5, 8, 2, 16, BF16), UNSUPPORTED), ((p, p, 2, 5, 8, 3, 23, BF16), INVALID),
                           ((p, p, 2, 5, 8, 3, 16, BF16), INVALID), ((p, p, 2, 0, 8, 3, 24, BF16), INVALID),
                           ((p, p, 2, 5, 0, 3, 24, BF16), INVALID), ((None, p, 2, 5, 8, 3, 24, BF16), INVALID),
                           ((p, p, -1, 5, 8, 3, 24, BF16), INVALID), ((p, p, 2, 5, 8, 3, 24, 9), INVALID)):
            assert fn(*args, None) == code, args
    assert h.ofa_tanh_dropout_fwd(p, p, 0, 0.5, 1, 0, None, F32, None) == 0                    # n == 0: nothing
    assert h.ofa_tanh_dropout_bwd(p, p, p, 0, 0.5, 1, 0, None, F32, None) == 0
    for args in ((p, p, 8, 1.0, 1, 0, None, F32), (p, p, 8, -0.1, 1, 0, None, F32), (p, p, -1, 0.5, 1, 0, None, F32),
                 (None, p, 8, 0.5, 1, 0, None, F32), (p, None, 8, 0.5, 1, 0, None, F32), (p, p, 8, 0.5, 1, 0, None, 5)):
        assert h.ofa_tanh_dropout_fwd(*args, None) == INVALID, args
    assert h.ofa_tanh_dropout_bwd(p, None, p, 8, 0.5, 1, 0, None, F32, None) == INVALID


def test_the_python_wrappers_refuse_before_the_library():
    from ofasys_amd import ops
    from ofasys_amd.lib import OfaError
    z = torch.zeros(2, 5, 8)
    with pytest.raises(ValueError, match="unknown reduction"):
        ops.tacotron2_loss(z, z, torch.zeros(2, 5, 1), z, torch.tensor([5, 3]), 1.0, "batchmean")
    with pytest.raises(OfaError, match="not on a GPU|must be one"):
        ops.tacotron2_eval(z, z, torch.zeros(2, 5, 1), z, torch.tensor([5, 3]))
