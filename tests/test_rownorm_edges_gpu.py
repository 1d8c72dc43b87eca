"""GPU: the row-normalisation kernels (csrc/layernorm.hip: LayerNorm and GELU+LayerNorm, forward and backward; csrc/join.hip: the fused
residual join, split-row and row-per-wave, forward and backward) on every route their dispatchers can launch, against the float64 oracle
of tests/rownorm_oracle.py.  Every element of every output is compared: 16-bit tensors within TOL eps of the reference relative to the
componentwise magnitude bound, exactly 0 where the bound is 0 (fp32 tensors: error / bound within G32); mean, rstd and the join's four
statistics against float64 within MEAN_TOL / RSTD_TOL.  Every output buffer holds NaN before the call.

What each test pins (the gaps the suite had):
  max|a-b| / max|b| at 2e-2, mean and rstd never read ... per element against the bound; mean and rstd against float64
  forward NV = 32 never ran, NV = 16 only in fp32 .......... both sides of every NV boundary in every dtype, 16384 columns included
  backward WPR 1 with NV 4 / 8, ragged parts ............... every (NV, WPR) the dispatcher reaches, plain and GELU, with and without dbias
  the fp32 six-waves-per-row GELU route .................... m = 384 vectors: 3072 columns in 16 bits, 1536 in fp32
  the prefetch ring's odd tail ............................. 1, 3, 513 and 1025 rows at m = 384: niter 1, 2 and 3
  a block's last live row, the second sweep ................ rpb - 1, rpb + 1, 256 rpb + 1 rows per WPR with dy = 64 in the seam row
  the join compared with kernels only ...................... against float64 in stages (y from x; z from y; dres; dx from dres)
  1536 columns, fp16, the flag space ....................... k = 1..6 in bf16 and fp16; dy / residual = None, want_dres, dx_colsum, offset_base,
                                                             keep = None with p > 0, every (LN_a, LN_b, p > 0) at k = 1..4
  the dropout mask ......................................... the stand-alone dropout kernel's, element for element; y == residual where dropped
  the forced forms of the debug library .................... one child process, the same oracle (tests/rownorm_gpu.py forced)
  refusals ................................................. asserted as exceptions, never launched
Run with -s for the worst figure per output and dtype."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import rownorm_gpu as rg
from tests import rownorm_oracle as ro

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]
DEV = rg.DEV
IDS = [ro.NAMES[d] for d in ro.DTYPES3]
WORST = {}                  # (output, dtype name) -> worst figure seen by this process, printed by every test (-s)


@pytest.fixture(scope="module")
def K():
    from ofasys_amd import kernels
    return kernels


def _report(title, family):
    print(f"\n{title}: " + ", ".join(f"{n} {d} {v:.3g}" for (n, d), v in sorted(WORST.get(family, {}).items())))


def _worst(family):
    return WORST.setdefault(family, {})


@pytest.mark.parametrize("dtype", ro.DTYPES3, ids=IDS)
def test_layernorm_forward(K, dtype):
    """ln_fwd_kernel<T, NV, GELU>: NV = 1 ... 32 on both sides of every boundary, one vector, 63 vectors, the widest row; 1, 3 and 5
    rows (a partial block of four waves); unit, offset and planted-column rows, one constant row; eps 1e-5 and 1e-3."""
    for case in ro.LN_FWD_CASES:
        b = ro.build_ln_fwd(case, dtype, DEV)
        rg.check("ln_fwd", ro.ln_fwd_figures(b, rg.run_ln_fwd(K, b), dtype), dtype, case.name, _worst("ln_fwd"))
    _report("LayerNorm forward", "ln_fwd")


def _ln_bwd(K, dtype, cases):
    for case in cases:
        b = ro.build_ln_bwd(case, dtype, DEV)
        rg.check("ln_bwd", ro.ln_bwd_figures(b, rg.run_ln_bwd(K, b), dtype), dtype, case.name, _worst("ln_bwd"))
    _report("LayerNorm backward", "ln_bwd")


@pytest.mark.parametrize("dtype", ro.DTYPES3, ids=IDS)
def test_layernorm_backward_shapes(K, dtype):
    """ln_bwd_kernel<T, NV, WPR, GELU>: every instantiation the dispatcher reaches (the table in tests/rownorm_oracle.py), rpb + 1 rows,
    with and without dres / dbias, fresh and accumulated parameter gradients."""
    _ln_bwd(K, dtype, [c for c in ro.LN_BWD_CASES if c.name.endswith("shape")])


@pytest.mark.parametrize("dtype", ro.DTYPES3, ids=IDS)
def test_layernorm_backward_rows(K, dtype):
    """Per waves-per-row route: 1, rpb - 1, rpb + 1 and 256 rpb + 1 rows (one live row in the second sweep); the prefetch ring at
    niter 1, 2, 3; dy = 64 in the last row, the last row of the first block iteration, the first row of the second sweep."""
    _ln_bwd(K, dtype, [c for c in ro.LN_BWD_CASES if not c.name.endswith("shape")])


@pytest.mark.parametrize("dtype", ro.DTYPES3, ids=IDS)
def test_join_flags_and_shapes(K, dtype):
    """join_fwd + join_bwd: k = 1 ... 6 row-per-wave shapes (fp32: the split-row kernels at the same columns), every (LN_a, LN_b, p > 0)
    at k = 1 ... 4, every split-row WPR with ragged parts, dy = None, residual = None, want_dres = False, dx_colsum, offset_base,
    keep = None with p > 0; gradients accumulated into pre-filled tensors."""
    for case in ro.JOIN_CASES:
        if case.rows <= 2048:
            keep = rg.join_case(K, case, dtype, _worst("join"))
            r = ro.join_route(ro.join_cols(case, dtype), dtype, True)
            assert (keep is not None) == (r.kind == "row" and case.p > 0), case.name
    _report("residual join", "join")


@pytest.mark.parametrize("dtype", ro.DTYPES3, ids=IDS)
def test_join_rows(K, dtype):
    """2049 and 4097 rows: two and three persistent iterations of the row-per-wave backward in flight (each waves-per-block /
    rows-ahead choice of join_bwd_row_launch); one live row in the second sweep of the split-row backward."""
    for case in ro.JOIN_CASES:
        if case.rows > 2048:
            rg.join_case(K, case, dtype, _worst("join"))
    _report("residual join, rows", "join")


def test_refusals_raise_before_any_launch(K):
    """Shapes the entry points refuse come back as exceptions from the wrappers: the output tensors stay NaN."""
    from ofasys_amd.lib import OfaError
    for dtype in ro.DTYPES3:
        N = ro.NVEC[dtype]
        mk = lambda *s: torch.ones(*s, dtype=dtype, device=DEV)          # noqa: E731
        cols = ro.FWD_REFUSED_M * N
        with pytest.raises(OfaError, match="exceeds"):
            K.layernorm_fwd(mk(2, cols), mk(cols), mk(cols))
        cols = ro.BWD_REFUSED_M * N                                      # the forward accepts, the backward refuses
        y, mean, rstd = K.layernorm_fwd(mk(2, cols), mk(cols), mk(cols))
        for gelu in (False, True):
            with pytest.raises(OfaError, match="too wide"):
                K.layernorm_bwd(mk(2, cols), mk(2, cols), mk(cols), mean, rstd, fuse_gelu=gelu)
    for dtype, cols in ro.JOIN_REFUSED:
        x = torch.ones(2, cols, dtype=dtype, device=DEV)
        g = torch.ones(cols, dtype=dtype, device=DEV)
        with pytest.raises(OfaError, match="join_fwd"):
            K.join_fwd(x, x, (g, g), None, 1e-5, 0.1, 1, 0, None)
        with pytest.raises(OfaError, match="join_bwd"):
            K.join_bwd(x, None, x, None, g, None, torch.ones(4, 2, device=DEV), 0.1, 1, 0, None, (g.clone(), g.clone(), None, None))
    torch.cuda.synchronize()


def test_forced_join_forms_against_the_oracle():
    """The debug library's forced forms (OFA_JOIN_FWD = 0 / 1, OFA_JOIN_BWD = 0 ... 3: split-row, and row-per-wave with 8 waves one row
    ahead, 4 waves two ahead, 8 waves two ahead; every valid pair, the row-per-wave forward under the split-row backward included;
    the child also shows that each switch changed the kernel that ran) on the reduced table -- one case per k and (LN_a, LN_b, p > 0), at 1, 7 and 2049 rows
    -- in one fresh child process, against the same float64 oracle.  tools/join_bench.py check stays beside it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dbg = os.path.join(root, "ofasys_amd", "libofasys_amd_dbg.so")
    assert os.path.exists(dbg), "the debug library is not built: make -C ofasys_amd/csrc debug"
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "rownorm_gpu.py"), "forced"], capture_output=True, text=True, timeout=600)
    line = next((ln for ln in reversed(r.stdout.splitlines()) if ln.startswith("{")), None)
    assert line is not None, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(line)
    print("\nforced join forms: " + ", ".join(f"{n} {v:.3g}" for n, v in out["worst"].items()))
    assert r.returncode == 0 and not out["failed"], out["failed"][:8]
