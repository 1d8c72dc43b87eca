"""GPU: MCD evaluation (csrc/dtw.hip, ofasys_amd/mcd.py) against plain float64 restatements written out here.

`dtw_ref` is the recurrence as a double loop: first row and column running sums, elsewhere d + min(left, up-left, up), the lowest code
(0 = left, 1 = up-left, 2 = up) on a tie, the path length carried along.  Integer data makes every fp32 sum exact, so those cases are bit
for bit.  Shapes sit at the kernel's seams: a tile is R = 4 rows; a lane's strip is C = 4 columns up to N = 1024, 8 up to 2048, 16 beyond
(distance form only); a wave is 64 strips (256 / 512 columns); the workgroup's full width is 256 strips (1024 columns at C = 4)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"
RAGGED = ((5, 257), (300, 64), (65, 129))
DIST_CASES = [((1, 1),), ((1, 7),), ((7, 1),), ((2, 2),), ((3, 3),), ((5, 5),), ((9, 255),), ((6, 257),), ((300, 64),), ((65, 129),),
              ((5, 1023),), ((3, 1025),), ((4, 2049),), RAGGED]


def dtw_ref(d):
    """float64 [M, N] -> (cum float64, bp int, len int)."""
    M, N = d.shape
    cum, bp, ln = np.zeros((M, N)), np.zeros((M, N), dtype=np.int64), np.zeros((M, N), dtype=np.int64)
    for i in range(M):
        for j in range(N):
            if i == 0 and j == 0:
                cum[i, j], bp[i, j], ln[i, j] = d[0, 0], 2, 1
                continue
            cands = [(cum[i, j - 1], 0, (i, j - 1))] if j > 0 else []
            if i > 0:
                cands += ([(cum[i - 1, j - 1], 1, (i - 1, j - 1))] if j > 0 else []) + [(cum[i - 1, j], 2, (i - 1, j))]
            best = min(cands, key=lambda c: (c[0], c[1]))
            cum[i, j], bp[i, j], ln[i, j] = d[i, j] + best[0], best[1], ln[best[2]] + 1
    return cum, bp, ln


def path_of(bp):
    i, j, out = bp.shape[0] - 1, bp.shape[1] - 1, []
    while True:
        out.append((i, j))
        if i == 0 and j == 0:
            return out[::-1]
        i, j = i - (bp[i, j] >= 1), j - (bp[i, j] <= 1)


@functools.lru_cache(maxsize=None)
def _int_distance(M, N):
    d = np.random.default_rng(1000 * M + N).integers(0, 3, (M, N)).astype(np.float64)
    return (d,) + dtw_ref(d)


def _pad(rows, width=None):
    out = np.zeros((len(rows), max(r.shape[0] for r in rows), width or max(r.shape[1] for r in rows)), dtype=np.float32)
    for b, r in enumerate(rows):
        out[b, :r.shape[0], :r.shape[1]] = r
    return torch.from_numpy(out).to(DEV)


def _shapes(case):
    return torch.tensor(case, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("case", DIST_CASES, ids=str)
def test_distance_form_is_exact(case):
    from ofasys_amd import kernels as K, mcd
    refs = [_int_distance(M, N) for M, N in case]
    dist, shapes = _pad([r[0] for r in refs]), _shapes(case)
    cum, bp, paths, pmap = mcd.batch_dynamic_time_warping(dist, shapes, pathmap=True)
    total, pathlen, _, _ = K.dtw(shapes, distance=dist)
    for b, ((M, N), (_, rc, rb, rl)) in enumerate(zip(case, refs)):
        assert np.array_equal(cum[b, :M, :N].cpu().numpy().astype(np.float64), rc), (b, "cumdist")
        assert np.array_equal(bp[b, :M, :N].cpu().numpy(), rb), (b, "backptr")
        assert float(total[b]) == rc[-1, -1] and int(pathlen[b]) == rl[-1, -1]
        p = paths[b].cpu().tolist()
        assert [tuple(x) for x in p] == path_of(rb) and len(p) == rl[-1, -1]
        # from the path alone: its ends and its steps
        assert p[0] == [0, 0] and p[-1] == [M - 1, N - 1]
        assert all((c[0] - a[0], c[1] - a[1]) in ((0, 1), (1, 1), (1, 0)) for a, c in zip(p, p[1:]))
        want = np.zeros((M, N), dtype=np.int64)
        want[tuple(np.array(p).T)] = 1
        assert np.array_equal(pmap[b, :M, :N].cpu().numpy(), want) and int(pmap[b].sum()) == len(p)


@functools.lru_cache(maxsize=None)
def _features(M, N, D, integer):
    rng = np.random.default_rng(7 + 1000 * M + N + D)
    draw = (lambda n: rng.integers(-3, 4, (n, D)).astype(np.float32)) if integer else (lambda n: rng.standard_normal((n, D)).astype(np.float32))
    return draw(M), draw(N)


def _l2(x1, x2):                                                         # float64, the difference formed directly
    return ((x1.astype(np.float64)[:, None, :] - x2.astype(np.float64)[None, :, :]) ** 2).sum(-1)


@pytest.mark.parametrize("D,ld", [(13, 13), (13, 16), (5, 8)])
@pytest.mark.parametrize("case", [((5, 257),), ((65, 1025),), RAGGED], ids=str)
def test_features_l2_is_exact(case, D, ld):
    from ofasys_amd import mcd
    feats = [_features(M, N, D, True) for M, N in case]
    res = mcd.batch_dtw_features(_pad([f[0] for f in feats], ld), _pad([f[1] for f in feats], ld), _shapes(case), metric="l2", D=D,
                                 return_path=True, return_backptr=True)
    for b, ((M, N), (x1, x2)) in enumerate(zip(case, feats)):
        rc, rb, rl = dtw_ref(_l2(x1, x2))
        got = (float(res.total[b]), int(res.pathlen[b]), int(res.nins[b]), int(res.ndel[b]))
        assert got == (rc[-1, -1], rl[-1, -1], rl[-1, -1] - M, rl[-1, -1] - N), (b, got)
        assert np.array_equal(res.backptr[b, :M, :N].cpu().numpy(), rb)
        assert [tuple(x) for x in res.path[0][b, :int(res.path[1][b])].cpu().tolist()] == path_of(rb)


@pytest.mark.parametrize("case", [((300, 64),), ((37, 1100),), RAGGED], ids=str)
def test_features_rms_within_the_derived_bound(case):
    """Every cell is a non-negative sum of at most M + N - 1 distances, each within a few ulp after subtract, square, sum, divide and sqrtf;
    min is monotone, so |total - ref| <= (M + N + 8 + D) 2^-23 ref."""
    from ofasys_amd import mcd
    D = 13
    feats = [_features(M, N, D, False) for M, N in case]
    res = mcd.batch_dtw_features(_pad([f[0] for f in feats], 16), _pad([f[1] for f in feats], 16), _shapes(case), metric="rms", D=D)
    for b, ((M, N), (x1, x2)) in enumerate(zip(case, feats)):
        ref = dtw_ref(np.sqrt(_l2(x1, x2) / D))[0][-1, -1]
        err, bound = abs(float(res.total[b]) - ref), (M + N + 8 + D) * 2.0 ** -23 * ref
        print(f"rms {case[b]}: total {float(res.total[b]):.6f} ref {ref:.6f} error {err:.3e} bound {bound:.3e}")
        assert err <= bound


def _mfcc_numpy(power, fn, dtype):
    from ofasys_amd import mcd
    bank, dct = mcd.htk_mel_filters(fn.sample_rate, fn.n_fft).astype(dtype), mcd.dct_table().astype(dtype)
    return np.log(power.astype(dtype) @ bank.T + dtype(1e-6)) @ dct.T


@pytest.mark.parametrize("sr", (22050, 16000))
def test_mfcc_rows_against_float64(sr):
    """The rule of tests/test_audio_features_gpu.py: the kernel's largest error against float64 is held to 4 x that of the same formula in
    float32 numpy (+ 1e-6 of the largest value).  Row 0 is all zero: the 1e-6 floor decides."""
    from ofasys_amd import kernels as K, mcd
    fn = mcd.MFCC(sr).to(DEV)
    assert fn.n_fft == {22050: 1102, 16000: 800}[sr]
    rng = np.random.default_rng(sr)
    power = (rng.standard_normal((7, fn.n_fft // 2 + 1)) ** 2 * 10.0 ** rng.uniform(-6, 2, (7, 1))).astype(np.float32)
    power[0] = 0.0
    got = K.mfcc_rows(torch.from_numpy(power).to(DEV), fn.filt_start, fn.filt_off, fn.filt_w, fn.dct).cpu().numpy()
    r64, r32 = _mfcc_numpy(power, fn, np.float64), _mfcc_numpy(power, fn, np.float32)
    e_k, e_32, scale = np.abs(got[:, :13] - r64).max(), np.abs(r32 - r64).max(), np.abs(r64).max()
    print(f"mfcc_rows sr={sr}: kernel {e_k / scale:.3e}, float32 numpy {e_32 / scale:.3e}, ratio {e_k / max(e_32, 1e-30):.3f}")
    assert not got[:, 13:].any() and e_k <= 4 * e_32 + 1e-6 * scale


def _mcd_numpy(y1, y2, sr, dtype):
    """(total, pathlen, M, N) of one pair through the whole chain in `dtype`: frames by hand, rfft, filters, log, DCT, rms, the double loop."""
    from ofasys_amd import mcd
    n_fft, hop = int(0.05 * sr), int(0.0125 * sr)
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)).astype(dtype)
    bank, dct = mcd.htk_mel_filters(sr, n_fft).astype(dtype), mcd.dct_table().astype(dtype)

    def feats(y):
        x = np.pad(y.astype(dtype), n_fft // 2, mode="reflect")
        f = np.stack([x[t * hop: t * hop + n_fft] for t in range(1 + len(y) // hop)]) * window
        spec = np.fft.rfft(f, axis=1)
        power = (spec.real ** 2 + spec.imag ** 2).astype(dtype)
        return np.log(power @ bank.T + dtype(1e-6)) @ dct.T
    x1, x2 = feats(y1), feats(y2)
    dist = np.sqrt(((x1[:, None, :] - x2[None, :, :]) ** 2).sum(-1) / dtype(13))
    cum, _, ln = dtw_ref(dist)
    return cum[-1, -1], int(ln[-1, -1]), x1.shape[0], x2.shape[0]


@functools.lru_cache(maxsize=None)
def _mcd_case():
    rng, sr = np.random.default_rng(3), 22050

    def wave(n):
        t = np.arange(n) / sr
        return (0.3 * np.sin(2 * np.pi * rng.uniform(100, 400) * t) + 0.1 * np.sin(2 * np.pi * rng.uniform(1000, 3000) * t)
                + 0.05 * rng.standard_normal(n)).astype(np.float32)
    y1, y2 = [wave(6615), wave(11025)], [wave(11025), wave(8000)]
    return y1, y2, [_mcd_numpy(a, b, sr, np.float64) for a, b in zip(y1, y2)], [_mcd_numpy(a, b, sr, np.float32) for a, b in zip(y1, y2)]


@pytest.mark.parametrize("normalize_type", [None, "len1", "len2", "path"])
def test_mel_cepstral_distortion_end_to_end(normalize_type):
    """Tolerance: the rms bound of the DTW above plus 4 x the gap of the same chain in float32 numpy, both computed here."""
    from ofasys_amd import batch_mel_cepstral_distortion
    y1, y2, r64, r32 = _mcd_case()
    rets = batch_mel_cepstral_distortion([torch.from_numpy(y) for y in y1], [torch.from_numpy(y) for y in y2], 22050, normalize_type)
    for (got, (L, M, N)), (t64, L64, M64, N64), (t32, _, _, _) in zip(rets, r64, r32):
        div = {None: 1, "len1": M64, "len2": N64, "path": L64}[normalize_type]
        tol = ((M64 + N64 + 8 + 13) * 2.0 ** -23 * t64 + 4 * abs(t32 - t64)) / div
        print(f"mcd {normalize_type} ({M}, {N}): got {got:.6f} ref {t64 / div:.6f} error {abs(got - t64 / div):.3e} tolerance {tol:.3e} path {L} / {L64}")
        assert (M, N) == (M64, N64) and abs(got - t64 / div) <= tol
        if normalize_type != "path":
            continue
        assert max(M, N) <= L <= M + N - 1


def test_valid_step_with_inference_reports_the_reference_keys(tmp_path):
    from oracle import recipe
    from ofasys_amd import Task
    from ofasys_amd.preprocessor import to_device
    from tests import speech_gen_case as C
    from tests.golden_util import load_golden
    from tests.test_speech_gen_gpu import _model
    golden = load_golden("speech_gen")
    mean, std = C.gcmvn_stats()
    np.savez(tmp_path / "gcmvn_stats.npz", mean=mean, std=std)
    model, d = _model("n1", torch.float32, golden=golden)
    tokens = C.source_tokens(len(d)).to(DEV)
    task = Task(name="tts", instruction="[TEXT:src] -> [AUDIO:fbank]", micro_batch_size=3)
    task.initialize(d)
    # threshold 2: nobody finishes, every hypothesis has 12 frames -- Griffin-Lim and the MFCC's reflect padding both need more than two
    args = '{"max_iter": 12, "eos_prob_threshold": 2.0, "stats_npz_path": "%s"' % (tmp_path / "gcmvn_stats.npz")
    rows = [{"src": f"sentence {i}", "fbank": {"fbank": recipe.floats(f"speech_gen.task.{i}", (4, C.RAW)), "fbank_lengths": 4}} for i in range(3)]
    task.add_dataset(rows, "valid")
    batch = to_device(task.get_sample("valid"), DEV)
    [s for s in batch["net_input"]["slots"] if s.is_src][0].value = tokens
    task.cfg.evaluation.generator_args = args + "}"
    with pytest.raises(ValueError, match="no vocoder"):
        task.valid_step_with_inference(model, batch)
    task.generator, task.cfg.audio.target_sr = None, 22050
    task.cfg.evaluation.generator_args = args + ', "vocoder": "griffin_lim", "spec_bwd_max_iter": 2}'
    hypos, losses = task.valid_step_with_inference(model, batch)
    assert len(hypos) == 3 and list(losses) == ["mcd_loss", "targ_frames", "pred_frames", "nins", "ndel"]
    frames = lambda w: 1 + w.numel() // 275                              # noqa: E731
    assert losses["targ_frames"] == sum(frames(h.targ_waveform) for h in hypos) and losses["pred_frames"] == sum(frames(h.waveform) for h in hypos)
    assert losses["nins"] - losses["ndel"] == losses["pred_frames"] - losses["targ_frames"]       # L - M - (L - N), summed
    assert losses["nins"] >= 0 and losses["ndel"] >= 0 and np.isfinite(losses["mcd_loss"]) and losses["mcd_loss"] > 0
