"""CPU: the Griffin-Lim vocoder's host side -- routing, the C ABI's shape, the served shapes, and the host-made tables.  librosa and
torchaudio are not installed, so the mel filters are held to their defining properties, not to librosa.filters.mel itself."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

FEATURES = dict(sample_rate=22050, n_fft=1024, win_len_t=1024 / 22050, hop_len_t=256 / 22050, n_mels=80, f_min=0, f_max=8000, window_fn="hann")


def test_get_vocoder_and_the_task_route_to_griffin_lim():
    from ofasys_amd import Dictionary, GriffinLimVocoder, Task
    from ofasys_amd.module.vocoder import get_vocoder
    args = SimpleNamespace(vocoder="griffin_lim", spec_bwd_max_iter=5, fp16=False)
    voc = get_vocoder(args, SimpleNamespace(config={"features": FEATURES}))
    assert isinstance(voc, GriffinLimVocoder) and (voc.n_fft, voc.win, voc.hop, voc.n_iter) == (1024, 1024, 256, 5)
    assert voc.out_len(40) == 256 * 39 and voc.pinv_t.shape == (80, 513) and voc.twiddle.shape == (512, 2)
    t = Task(name="tts", instruction="[TEXT:src] -> [AUDIO:fbank]")
    t.initialize(Dictionary())
    g = t.build_speech_generator(vocoder="griffin_lim", vocoder_features={"n_fft": 512, "win_length": 400, "hop_length": 100})
    assert isinstance(g.vocoder, GriffinLimVocoder) and (g.vocoder.n_fft, g.vocoder.win, g.vocoder.hop, g.vocoder.n_iter) == (512, 400, 100, 8)
    assert t.build_speech_generator(max_iter=40).vocoder is None
    with pytest.raises(ValueError, match="unknown keys"):
        t.build_speech_generator(vocoder="griffin_lim", vocoder_features={"hop": 100})


def test_prototypes_and_served_shapes():
    from ofasys_amd import kernels as K
    from ofasys_amd.lib import lib
    for name, count in {"ofa_griffin_lim_run": 3, "ofa_griffin_lim_project": 14, "ofa_griffin_lim_inverse": 14, "ofa_griffin_lim_specgram": 8}.items():
        assert len(lib().protos[name][1]) == count, name
    # four times the halo ceil(n_fft / hop) - 1 (recomputation 1.25 x); without overlap 4 frames, or what the LDS leaves
    assert [K.griffin_lim_run(*s) for s in ((256, 256, 64), (256, 255, 63), (256, 256, 256), (1024, 1024, 256), (2048, 2048, 512), (2048, 2048, 2048))] == \
        [12, 16, 4, 12, 12, 3]
    assert K.griffin_lim_run(1000, 1000, 250) == 0 and K.griffin_lim_run(1024, 1024, 0) == 0 and K.griffin_lim_run(1024, 1025, 256) == 0
    assert K.griffin_lim_run(128, 128, 32) == 0 and K.griffin_lim_run(4096, 4096, 1024) == 0
    rc = lib().cdll.ofa_griffin_lim_project(None, None, None, None, None, 0, None, None, 0, 4, 1000, 1000, 250, None)
    assert rc == 2 and lib().cdll.ofa_last_error().decode().startswith("griffin_lim_project")       # OFA_ERR_UNSUPPORTED, before any launch


@pytest.mark.parametrize("n_frames,hop,win,n_fft", [(4, 64, 256, 256), (9, 63, 255, 256), (5, 256, 256, 256), (40, 256, 1024, 1024), (1, 100, 400, 512)])
def test_window_sum_square_is_the_reference_loop(n_frames, hop, win, n_fft):
    from ofasys_amd.module.vocoder import get_window, window_sum_square
    window = get_window(torch.hann_window, n_fft, win)
    assert window.shape == (n_fft,) and float(window[: (n_fft - win) // 2].abs().sum()) == 0.0 and float(window[(n_fft - win) // 2 + 1]) > 0
    w_sq = window ** 2                                                   # GriffinLim.get_window_sum_square, as written there
    n = n_fft + hop * (n_frames - 1)
    x = torch.zeros(n, dtype=torch.float32)
    for i in range(n_frames):
        ofst = i * hop
        x[ofst: min(n, ofst + n_fft)] += w_sq[: max(0, min(n_fft, n - ofst))]
    assert torch.equal(window_sum_square(window, n_frames, hop), x)


def test_mel_filters_have_slaney_properties():
    from ofasys_amd.module.vocoder import _hz_to_mel, _mel_to_hz, mel_filters
    assert float(_hz_to_mel(1000.0)) == 15.0 and abs(float(_mel_to_hz(_hz_to_mel(4321.0))) - 4321.0) < 1e-9 and float(_hz_to_mel(500.0)) == 7.5
    assert abs(float(_hz_to_mel(6400.0)) - 42.0) < 1e-12                # 27 mels per factor 6.4 above 1000 Hz
    f = mel_filters(22050, 1024, 80, 0, 8000)
    assert f.shape == (80, 513) and f.dtype == torch.float32 and float(f.min()) >= 0.0 and bool((f.sum(1) > 0).all())
    # Slaney's normalisation: a triangle over [lo, hi] has height 2 / (hi - lo), area 1.  Sampled every df Hz, the sum misses the integral of
    # a piecewise-linear function by at most df^2 / 8 per unit of slope change at each of its three kinks.
    pts, df = _mel_to_hz(np.linspace(_hz_to_mel(0), _hz_to_mel(8000), 82)), 22050 / 1024
    for i in range(80):
        up, down = 2 / (pts[i + 2] - pts[i]) / (pts[i + 1] - pts[i]), 2 / (pts[i + 2] - pts[i]) / (pts[i + 2] - pts[i + 1])
        assert abs(float(f[i].double().sum()) * df - 1.0) <= df ** 2 / 8 * 2 * (up + down) + 1e-6, i
        assert float(f[i].max()) <= 2 / (pts[i + 2] - pts[i]) * (1 + 1e-6)
        on = f[i].nonzero().flatten() * df
        assert float(on.min()) > pts[i] - 1e-6 and float(on.max()) < pts[i + 2] + 1e-6


def test_short_utterances_are_refused_at_the_call():
    from ofasys_amd import GriffinLimVocoder
    voc = GriffinLimVocoder(22050, 256, 64, 256, 80, 0, 8000, torch.hann_window, spec_bwd_max_iter=2)
    with pytest.raises(ValueError, match="too few to reflect-pad"):      # 64 * 2 = 128 samples = n_fft / 2: torch's reflect pad refuses it too
        voc(torch.zeros(3, 80))
    with pytest.raises(ValueError, match="too few to reflect-pad"):
        voc(torch.zeros(2, 6, 80), lengths=[6, 3])
    with pytest.raises(ValueError, match="power of two"):
        GriffinLimVocoder(22050, 1000, 250, 1000, 80, 0, 8000, "hann")
