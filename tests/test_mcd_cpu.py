"""CPU: the host side of MCD evaluation (ofasys_amd/mcd.py, csrc/dtw.hip's entry points) -- the C ABI's shape, the refusals before any
launch, and the host-made mel filters and DCT table against their formulas."""
import math

import numpy as np
import pytest
import torch

from ofasys_amd import kernels as K, mcd
from ofasys_amd.lib import OfaError, lib


def test_header_declares_and_library_exports():
    for name, count in {"ofa_dtw": 17, "ofa_dtw_backtrace": 8, "ofa_mfcc_rows": 13, "ofa_dtw_strip": 3}.items():
        assert len(lib().protos[name][1]) == count and hasattr(lib().cdll, name), name
    assert [K.dtw_strip(True, n) for n in (1, 1024, 1025, 2048, 2049)] == [4, 4, 8, 8, 0]
    assert [K.dtw_strip(False, n) for n in (1024, 2049, 4096)] == [4, 16, 16] and K.dtw_strip(False, 2048, 4) == 0


@pytest.mark.parametrize("args,rc,words", [
    ((None,) * 8 + (1, 30, 10, 17, 17, 1, 0, 0, None), 2, ("D=17", "16")),
    ((None,) * 8 + (1, 3000, 10, 13, 16, 1, 0, 0, None), 2, ("2048", "maxM=3000", "maxN=10")),
    ((None,) * 8 + (1, 30, 10, 13, 16, 1, 0, 1, None), 2, ("dtype=1",)),
    ((None,) * 8 + (1, 30, 10, 13, 16, 1, 16, 0, None), 2, ("strip=16",))])
def test_the_entry_point_refuses_before_any_launch(args, rc, words):
    assert lib().cdll.ofa_dtw(*args) == rc
    msg = lib().cdll.ofa_last_error().decode()
    assert msg.startswith("dtw:") and all(w in msg for w in words), msg


def test_the_wrappers_refuse_with_the_offending_numbers():
    shapes = torch.zeros(1, 2, dtype=torch.int32)
    for kw, words in ((dict(x1=torch.zeros(1, 4, 17), x2=torch.zeros(1, 5, 17)), ("D=17", "16")),
                      (dict(x1=torch.zeros(1, 2049, 13), x2=torch.zeros(1, 5, 13)), ("2048", "maxM=2049", "maxN=5")),
                      (dict(distance=torch.zeros(1, 5, 4097)), ("4096", "maxN=4097")),
                      (dict(distance=torch.zeros(1, 5, 8, dtype=torch.bfloat16)), ("fp32", "bfloat16")),
                      (dict(x1=torch.zeros(1, 4, 13), x2=torch.zeros(1, 5, 13), metric="l1"), ("'l1'",))):
        with pytest.raises(OfaError) as e:
            K.dtw(shapes, **kw)
        assert all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(OfaError, match="fp32 only, got torch.float16"):
        K.mfcc_rows(torch.zeros(2, 401, dtype=torch.float16), *[torch.zeros(1)] * 4)
    with pytest.raises(ValueError, match="normalize_type len3 not supported"):
        mcd.batch_mel_cepstral_distortion([torch.zeros(900)], [torch.zeros(900)], 22050, normalize_type="len3")
    with pytest.raises(ValueError, match="551 samples is too short to reflect-pad by n_fft // 2 = 551"):
        mcd.MFCC(22050)(torch.zeros(551))


def test_tables_follow_their_formulas():
    fb = mcd.htk_mel_filters(22050, 1102)
    assert fb.shape == (80, 552) and fb.dtype == np.float64 and fb.min() >= 0.0 and fb.max() <= 1.0
    assert (fb > 0).sum(0).max() <= 2 and (fb > 0).sum(1).min() >= 1 and not fb[:, 0].any()      # bin 0 is 0 Hz, below f_min = 20
    # by hand: filter 0 rises from 20 Hz to the second of 82 points equally spaced in mel between mel(20) and mel(11025), then falls to the third
    mel, inv = lambda f: 2595.0 * math.log10(1.0 + f / 700.0), lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)   # noqa: E731
    p = [inv(mel(20.0) + k * (mel(11025.0) - mel(20.0)) / 81.0) for k in range(3)]
    f2 = 2 * 11025.0 / 551.0                                                                     # bin 2 of linspace(0, 11025, 552)
    assert p[0] < f2 < p[2]
    assert fb[0, 2] == pytest.approx(min((f2 - p[0]) / (p[1] - p[0]), (p[2] - f2) / (p[2] - p[1])), rel=1e-12)
    dct = mcd.dct_table()
    assert dct.shape == (13, 80) and np.abs(dct @ dct.T - np.eye(13)).max() < 1e-14
    assert dct[0, 5] == pytest.approx(1.0 / math.sqrt(80.0), rel=1e-14)
    assert dct[3, 7] == pytest.approx(math.cos(math.pi / 80.0 * 7.5 * 3.0) * math.sqrt(2.0 / 80.0), rel=1e-14)
    fn = mcd.MFCC(16000)
    assert (fn.n_fft, fn.hop, fn.num_frames(4800), fn.window.numel()) == (800, 200, 25, 800) and fn.filt_w.numel() < 401 * 3
