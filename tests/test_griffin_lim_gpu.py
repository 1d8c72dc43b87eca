"""GPU: the Griffin-Lim kernels (csrc/griffin_lim.hip) and their way to the user, against `Restatement`: the reference's own formulas
(module/vocoder.py:52-103, utils/audio_utils.py:202-251) in torch on the CPU -- dense bases from np.fft.fft(np.eye(n_fft)) and
torch.pinverse, reflect pad, conv1d, atan2, cos / sin, conv_transpose1d, the window-sum-square loop, the scaling and the trims.

No tolerance is a fitted constant: a per-element test runs the restatement in float64 AND in float32 and holds the kernel's max-abs error
to 4 x the float32 restatement's own error against float64 (an FFT sums in another order than a dense product), both over max |w64|, plus
a floor of 1e-6.  The ratios are printed (profiles/griffin_lim_parity.txt keeps one run of them)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = "cuda"


class Restatement:
    def __init__(self, n_fft, win, hop, dtype):
        from ofasys_amd.module.vocoder import get_window
        self.n_fft, self.hop, self.dtype = n_fft, hop, dtype
        basis = np.fft.fft(np.eye(n_fft))
        basis = torch.from_numpy(np.vstack([np.real(basis[: n_fft // 2 + 1]), np.imag(basis[: n_fft // 2 + 1])])).to(dtype)
        self.window = get_window(torch.hann_window, n_fft, win).to(dtype)
        self.fwd = basis.unsqueeze(1) * self.window
        self.inv = torch.pinverse(n_fft / hop * basis).T[:, None, :] * self.window

    def stft(self, w):                                                   # [L] -> magnitude, phase [K, T]
        x = F.pad(w.to(self.dtype)[None, None], (self.n_fft // 2, self.n_fft // 2), mode="reflect")
        x = F.conv1d(x, self.fwd, stride=self.hop)[0]
        re, im = x[: self.n_fft // 2 + 1], x[self.n_fft // 2 + 1:]
        return torch.sqrt(re ** 2 + im ** 2), torch.atan2(im, re)

    def inverse(self, S, phase):                                         # [K, T] each -> [hop (T - 1)]
        S, phase = S.to(self.dtype), phase.to(self.dtype)
        x = F.conv_transpose1d(torch.cat([S * torch.cos(phase), S * torch.sin(phase)])[None], self.inv, stride=self.hop)[0, 0]
        w_sq, n = self.window ** 2, x.numel()
        wss = torch.zeros(n, dtype=self.dtype)
        for i in range(S.shape[1]):
            wss[i * self.hop: min(n, i * self.hop + self.n_fft)] += w_sq[: max(0, min(self.n_fft, n - i * self.hop))]
        nz = wss > 1.1754944e-38
        x[nz] /= wss[nz]
        x *= self.n_fft / self.hop
        return x[self.n_fft // 2: -(self.n_fft // 2)]

    def project(self, w, S):
        return self.inverse(S, self.stft(w)[1])

    def run(self, S, phase, n_iter):
        w = self.inverse(S, phase)
        for _ in range(n_iter):
            w = self.project(w, S)
        return w


def _vocoder(n_fft, win, hop, n_iter=32):
    from ofasys_amd import GriffinLimVocoder
    return GriffinLimVocoder(22050, win, hop, n_fft, 80, 0, 8000, "hann", spec_bwd_max_iter=n_iter).to(DEV)


def _within(tag, got, w64, w32):
    """max |got - w64| <= 4 max |w32 - w64| + 1e-6 max |w64|, every utterance of the batch alone."""
    scale = max(float(w.abs().max()) for w in w64)
    e_k = max(float((g.double().cpu() - w).abs().max()) for g, w in zip(got, w64)) / scale
    e_32 = max(float((v.double() - w).abs().max()) for v, w in zip(w32, w64)) / scale
    print(f"{tag}: kernel {e_k:.3e}, float32 restatement {e_32:.3e}, ratio {e_k / max(e_32, 1e-30):.3f}")
    assert e_k <= 4 * e_32 + 1e-6


# (n_fft, win, hop, frames of every utterance given the run R): the shortest utterance reflect padding admits; run seams, halo frames and a
# ragged batch in one launch; a short window padded unevenly with a hop that divides nothing; no overlap (the periodic hann window is 0 at
# every frame start: the window-sum-square guard); the configuration's own size
CASES = [(256, 256, 64, lambda R: [4]), (256, 256, 64, lambda R: [R + 1, 2 * R + 3, 7]), (256, 255, 63, lambda R: [9]),
         (256, 256, 256, lambda R: [5]), (1024, 1024, 256, lambda R: [R + 2])]
IDS = ["shortest", "seams-ragged", "win255-hop63", "no-overlap", "config"]


@pytest.mark.parametrize("which", ("project", "inverse"))
@pytest.mark.parametrize("n_fft,win,hop,frames_of", CASES, ids=IDS)
def test_step_per_element(n_fft, win, hop, frames_of, which):
    from ofasys_amd import kernels as K
    frames = frames_of(K.griffin_lim_run(n_fft, win, hop))
    B, T, Kf, gen = len(frames), max(frames), n_fft // 2 + 1, torch.Generator().manual_seed(n_fft + hop)
    w = torch.randn(B, hop * (T - 1), generator=gen)
    S = torch.rand(B, T, Kf, generator=gen) + 0.1
    S[:, 1:3, 5:40] = 0.0
    phase = (torch.rand(B, T, Kf, generator=gen) * 2 - 1) * np.pi
    voc = _vocoder(n_fft, win, hop)
    tables = voc.tables(T, frames if B > 1 else None, DEV)
    src = w if which == "project" else phase
    got = getattr(K, "griffin_lim_" + which)(src.to(DEV), S.to(DEV), *tables)
    assert got.shape == (B, hop * (T - 1)) and got.dtype == torch.float32
    refs = {}
    for dtype in (torch.float64, torch.float32):
        r = Restatement(n_fft, win, hop, dtype)
        refs[dtype] = [r.project(w[b, :hop * (t - 1)], S[b, :t].t()) if which == "project" else r.inverse(S[b, :t].t(), phase[b, :t].t())
                       for b, t in enumerate(frames)]
    _within(f"{which} n_fft={n_fft} win={win} hop={hop} frames={frames}", [got[b, :hop * (t - 1)] for b, t in enumerate(frames)],
            refs[torch.float64], refs[torch.float32])
    for b, t in enumerate(frames):
        assert float(got[b, hop * (t - 1):].abs().sum()) == 0.0


@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("fp32", "bf16"))
def test_specgram_per_element(dtype):
    from ofasys_amd import kernels as K
    voc = _vocoder(1024, 1024, 256)
    x = torch.randn(5, 80, generator=torch.Generator().manual_seed(3)).to(dtype)
    got = K.griffin_lim_specgram(x.to(DEV), voc.pinv_t)
    pinv = voc.pinv_t.t().cpu()
    want = (pinv.double() @ x.double().exp().t()).clamp(min=0).t()
    assert got.shape == (5, 513) and got.dtype == torch.float32 and float(got.min()) >= 0.0
    _within(f"specgram {dtype}", [got], [want], [(pinv @ x.float().exp().t()).clamp(min=0).t()])


def test_vocoder_converges_as_float64_does():
    """The configuration's defaults, T = 40, 32 iterations from supplied angles: the spectral convergence || |STFT(w)| - S || / || S ||
    (measured by the float64 restatement) is at most 1.05 x the float64 restatement's on the same S -- fp32 trajectories diverge over
    32 iterations; were the float32 restatement itself further off, the margin would be twice its excess, and the print says so."""
    voc, gen = _vocoder(1024, 1024, 256), torch.Generator().manual_seed(7)
    x = torch.randn(2, 40, 80, generator=gen) - 3.0
    angles = (torch.rand(2, 513, 40, generator=gen) * 2 - 1) * np.pi
    lens = [40, 23]
    got = voc(x.to(DEV), lengths=lens, angles=angles)
    assert got.shape == (2, 1, 256 * 39) and got.dtype == torch.float32
    assert torch.equal(got, voc(x.to(DEV), lengths=lens, angles=angles))                     # equal inputs, equal bits
    for b, t in enumerate(lens):                                                              # the ragged batch = its utterances alone
        alone = voc(x[b, :t].to(DEV), angles=angles[b, :, :t])
        assert alone.shape == (1, 256 * (t - 1)) and torch.equal(got[b, :, :256 * (t - 1)], alone) and float(got[b, 0, 256 * (t - 1):].abs().sum()) == 0.0
    from ofasys_amd import kernels as K
    S = K.griffin_lim_specgram(x[0].to(DEV), voc.pinv_t).cpu().t()                            # [513, 40]: the input all three share
    r64, r32 = Restatement(1024, 1024, 256, torch.float64), Restatement(1024, 1024, 256, torch.float32)

    def sc(w):
        return float((r64.stft(w)[0] - S.double()).norm() / S.double().norm())
    c_k, c_64, c_32 = sc(got[0, 0].cpu()), sc(r64.run(S, angles[0], 32)), sc(r32.run(S, angles[0], 32))
    margin = max(1.05, 1.0 + 2.0 * (c_32 / c_64 - 1.0))
    print(f"spectral convergence after 32 iterations: kernel {c_k:.6f}, float64 {c_64:.6f}, float32 {c_32:.6f}; margin {margin:.4f}")
    assert c_k <= margin * c_64


def test_speech_generator_vocodes_by_out_len():
    from ofasys_amd import AutoRegressiveSpeechGenerator, Dictionary
    g = AutoRegressiveSpeechGenerator(Dictionary(), vocoder=_vocoder(256, 256, 64, n_iter=2))
    lens = torch.tensor([6, 4])
    wav = g._vocode(torch.randn(2, 6, 80, generator=torch.Generator().manual_seed(1)).to(DEV), lens)
    assert [tuple(w.shape) for w in wav] == [(64 * 5,), (64 * 3,)] and all(w.dtype == torch.float32 and not w.is_cuda and float(w.abs().max()) > 0
                                                                           for w in wav)
