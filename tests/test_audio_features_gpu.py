"""GPU: log-mel feature extraction and utterance CMVN (csrc/audio_features.hip) and their way to the user, against `restate`: the two
front ends in plain numpy -- framing, DC removal, pre-emphasis, window, a dense DFT product, the dense filter bank -- run in float64 AND
in float32.  No tolerance is a fitted constant: the kernel's error against float64 is held to 4 x the float32 restatement's own (an FFT
sums in another order than a dense product) plus 1e-6, in two measures:
    linear  max |exp(got) - E64| over the frame's largest E64
    log     max |got - log E64| over the elements with E64 >= 1e-6 x the frame's largest; those left out must be under 1 % of all
The ratios are printed (profiles/audio_features_parity.txt keeps one run of them)."""
import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"


def restate(ext, bank, wav, dtype):
    """Mel energies E [T, n_mels] of one utterance (1-D, int16 scale) in `dtype`."""
    N, win, shift, T = ext.n_fft, ext.win, ext.shift, ext.num_frames(len(wav))
    window, x = ext.window.cpu().numpy().astype(dtype), np.asarray(wav).astype(dtype)
    if ext.kind == "kaldi":
        f = np.stack([x[t * shift: t * shift + win] for t in range(T)])
        f = f - f.mean(1, keepdims=True)
        f = (f - dtype(0.97) * np.concatenate([f[:, :1], f[:, :-1]], axis=1)) * window[:win]
        f = np.pad(f, ((0, 0), (0, N - win)))
    else:
        x = np.pad(x * dtype(2.0 ** -15), N // 2, mode="reflect")
        f = np.stack([x[t * shift: t * shift + N] for t in range(T)]) * window
    ang = 2.0 * np.pi * np.outer(np.arange(N), np.arange(N // 2 + 1)) / N
    re, im = f @ np.cos(ang).astype(dtype), f @ np.sin(ang).astype(dtype)
    power = re * re + im * im
    return (power if ext.kind == "kaldi" else np.sqrt(power)) @ bank.astype(dtype).T


def _banks(ext):
    from ofasys_amd.module.audio_features import kaldi_mel_banks
    from ofasys_amd.module.vocoder import mel_filters
    if ext.kind == "kaldi":
        return kaldi_mel_banks(ext.sample_rate, ext.n_fft, ext.n_mels)
    return mel_filters(ext.sample_rate, ext.n_fft, ext.n_mels, 0, 8000).double().numpy()


def _waves(lens, seed):
    rng = np.random.default_rng(seed)                                    # the offset makes the DC removal matter
    return [(rng.standard_normal(n) * 3000.0 + 500.0).astype(np.float32) for n in lens]


def _measures(rows, E64, stats=None):
    """(linear, log, share left out) of log-mel rows [T, n_mels] against E64; stats: the (mean, std) epilogue the rows went through."""
    rows = rows.astype(np.float64) if stats is None else rows.astype(np.float64) * stats[1] + stats[0]
    top = E64.max(1, keepdims=True)
    keep = E64 >= 1e-6 * top
    return (np.abs(np.exp(rows) - E64) / top).max(), np.abs(rows - np.log(np.where(keep, E64, 1.0)))[keep].max(), 1.0 - keep.mean()


def _kaldi(sr, n_mels):
    from ofasys_amd import LogMelExtractor
    return LogMelExtractor.kaldi(sr, n_mels).to(DEV)


def _tts(n_fft, win, hop, stats=None):                                  # (40 filters at n_fft = 256: with 80 the narrowest would hold no bin)
    from ofasys_amd import LogMelExtractor
    return LogMelExtractor.tts(22050, win, hop, n_fft, 80 if n_fft > 256 else 40, 0, 8000, "hann", stats).to(DEV)


# (extractor, sample counts given the run R): one frame; workgroup seams, zeroed tail rows and trailing samples that no frame takes, in a
# ragged batch; N = 256 with fewer filters than lanes and an odd row pitch; an odd window in N = 1024 with more than 64 filters; an uneven
# window pad with a hop that divides nothing; the configuration's own size with the global-CMVN epilogue; the shortest reflect padding admits
CASES = {"kaldi16k-one-frame": (lambda p: _kaldi(16000, 80), lambda R: [400]),
         "kaldi16k-seams-ragged": (lambda p: _kaldi(16000, 80), lambda R: [400, 400 + 160 * R + 37, 400 + 160 * (2 * R + 2)]),
         "kaldi8k-23mels": (lambda p: _kaldi(8000, 23), lambda R: [4003, 2001]),
         "kaldi22k-win551": (lambda p: _kaldi(22050, 80), lambda R: [11025, 5513]),
         "tts-256-255-63": (lambda p: _tts(256, 255, 63), lambda R: [2999, 1500]),
         "tts-1024-cmvn": (lambda p: _tts(1024, 1024, 256, p), lambda R: [11025, 6000]),
         "tts-shortest": (lambda p: _tts(256, 256, 64), lambda R: [129])}


@pytest.mark.parametrize("case", CASES)
def test_logmel_per_element(case, tmp_path):
    from ofasys_amd import kernels as K
    rng = np.random.default_rng(5)
    stats = (rng.standard_normal(80) - 5.0, rng.random(80) + 0.5)
    np.savez(tmp_path / "stats.npz", mean=stats[0], std=stats[1])
    ext = CASES[case][0](str(tmp_path / "stats.npz"))
    stats = None if ext.mean is None else (ext.mean.double().cpu().numpy(), ext.std.double().cpu().numpy())
    lens = CASES[case][1](K.logmel_run(ext.kind, ext.n_fft, ext.win, ext.shift))
    waves = _waves(lens, len(case))
    batch = torch.zeros(len(lens), max(lens))
    for b, w in enumerate(waves):
        batch[b, :len(w)] = torch.from_numpy(w)
    got, frames = ext(batch, lens if len(lens) > 1 else None)
    assert got.shape == (len(lens), max(frames), ext.n_mels) and got.dtype == torch.float32 and frames.tolist() == [ext.num_frames(n) for n in lens]
    bank, worst = _banks(ext), np.zeros((2, 3))
    for b, (w, T) in enumerate(zip(waves, frames.tolist())):
        alone, _ = ext(torch.from_numpy(w))                              # the ragged batch = its utterances alone, bit for bit
        assert torch.equal(got[b, :T], alone[0]) and float(got[b, T:].abs().sum()) == 0.0
        E64, E32 = restate(ext, bank, w, np.float64), restate(ext, bank, w, np.float32)
        log32 = np.log(np.maximum(E32, np.float32(1e-5 if ext.kind == "tts" else 1.1920929e-07)))
        if stats is not None:                                            # (the epilogue in float32 as well)
            log32 = (log32 - stats[0].astype(np.float32)) / stats[1].astype(np.float32)
        worst = np.maximum(worst, [_measures(got[b, :T].cpu().numpy(), E64, stats), _measures(log32, E64, stats)])
    (lin_k, log_k, out_k), (lin_32, log_32, out_32) = worst
    print(f"{case} frames={frames.tolist()}: linear kernel {lin_k:.3e} float32 {lin_32:.3e} ratio {lin_k / max(lin_32, 1e-30):.3f}; "
          f"log kernel {log_k:.3e} float32 {log_32:.3e} ratio {log_k / max(log_32, 1e-30):.3f}; left out {out_k:.4%}")
    assert out_k < 0.01
    assert lin_k <= 4 * lin_32 + 1e-6 and log_k <= 4 * log_32 + 1e-6


@pytest.mark.parametrize("kind,floor", [("kaldi", 1.1920929e-07), ("tts", 1e-5)])
def test_a_silent_frame_gives_the_floor(kind, floor):
    ext = _kaldi(16000, 80) if kind == "kaldi" else _tts(256, 256, 64)
    got, frames = ext(torch.zeros(600))
    assert frames.tolist() == [ext.num_frames(600)] and got.shape[1] > 1
    assert float((got / np.log(floor) - 1.0).abs().max()) <= 1e-6


@pytest.mark.parametrize("flags", [(True, True), (True, False), (False, True)])
def test_utterance_cmvn_per_element(flags):
    """The float64 formula of UtteranceCMVN against the kernel and against the same formula in float32 numpy: T = 1 (variance 0: the std
    floor), an utterance of 0 frames, rows past the frame count."""
    from ofasys_amd import kernels as K
    frames, F = [1, 0, 37, 300], 80
    x = torch.randn(len(frames), max(frames), F, generator=torch.Generator().manual_seed(2)) * 2.0 - 5.0
    for b, t in enumerate(frames):
        x[b, t:] = 0.0

    def formula(v):
        mean, sq = v.mean(0), (v ** 2).sum(0)
        v = v - mean if flags[0] else v
        return v / np.sqrt(np.maximum(sq / v.shape[0] - mean ** 2, v.dtype.type(1e-10))) if flags[1] else v
    got = K.utterance_cmvn(x.to(DEV), torch.tensor(frames, dtype=torch.int32, device=DEV), *flags).cpu()
    e_k = e_32 = scale = 0.0
    for b, t in enumerate(frames):
        assert torch.equal(got[b, t:], x[b, t:])
        if t:
            r64 = formula(x[b, :t].double().numpy())
            scale = max(scale, np.abs(r64).max())
            e_k, e_32 = max(e_k, np.abs(got[b, :t].double().numpy() - r64).max()), max(e_32, np.abs(formula(x[b, :t].numpy()) - r64).max())
    print(f"utterance_cmvn {flags}: kernel {e_k / scale:.3e}, float32 formula {e_32 / scale:.3e}")
    assert e_k / scale <= 4 * e_32 / scale + 1e-6
    alone = K.utterance_cmvn(x[2:3, :37].contiguous().to(DEV), None, *flags).cpu()
    assert torch.equal(alone[0], got[2, :37])


@pytest.mark.parametrize("side", ["source", "target"])
def test_a_task_collates_wav_values_as_it_collates_their_frames(side):
    from ofasys_amd import Dictionary, Task
    template, col = ("[AUDIO:wav] -> [TEXT:text]", "wav") if side == "source" else ("[TEXT:text] -> [AUDIO:fbank,n_frames_per_step=2]", "fbank")
    task = Task(name=side, instruction=template)
    task.cfg.audio.utterance_cmvn, task.cfg.audio.target_sr = True, 16000 if side == "source" else 22050
    task.initialize(Dictionary())
    ext = task.general_preprocess.name2pre["audio"].extractor(side == "source").to(DEV)
    waves = _waves([5000, 3200, 7013], 11)
    ready = []
    for w in waves:
        feats, frames = ext(torch.from_numpy(w))
        ready.append({"fbank": feats[0].cpu().numpy(), "fbank_lengths": int(frames[0])})
    a = task.collate([{"text": "hello world", col: {"wav": w}} for w in waves])
    b = task.collate([{"text": "hello world", col: r} for r in ready])
    sa, sb = ([s for s in c["net_input"]["slots"] if s.modality.name == "AUDIO"][0].value for c in (a, b))
    assert torch.equal(sa["fbank"].cpu(), sb["fbank"]) and torch.equal(sa["fbank_lengths"], sb["fbank_lengths"]) and sa["fbank"].shape[1] > 1
    if side == "target":
        assert torch.equal(a["target"].cpu(), b["target"]) and torch.equal(a["target_lengths"], b["target_lengths"]) and a["ntokens"] == b["ntokens"]
        assert torch.equal(a["net_target"]["slots"][0].value["fbank"].cpu(), b["target"]) and a["target"].shape[2] == 160
