"""CPU: the reference scans the harmonic phases with an fp32 cumsum (generator.py:148); cv_hift_source computes the exact (fp64) phase.
The two are different quantities: their distance is the reference's own rounding, which grows with the running sum.  This pins how far
apart they may be, so that the GPU tests can hold the kernel to the fp64 scan and the goldens (fp32 scan) to a derived bound."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helpers as H  # noqa: E402

from cosyvoice_amd.config import HiftConfig  # noqa: E402
from oracle import hift as oh  # noqa: E402


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("T", [20, 500, 1000])
def test_fp32_scan_stays_within_one_ulp_of_the_running_sum(T, seed):
    """HiftConfig.v2(), uniform 80 - 400 Hz f0, phase_vec of draw_source_randoms(seed=5), noise zeroed: measured L-inf between the fp32-scan
    and the fp64-scan sine waves 1.9e-5 / 6.1e-4 / 1.2e-3 at 20 / 500 / 1000 frames against bounds 3.8e-5 / 1.2e-3 / 2.5e-3 (seed 0)."""
    cfg = HiftConfig.v2()
    torch.manual_seed(seed)
    f0 = torch.rand(1, T) * 320 + 80
    S = T * cfg.total_upsample
    f0_up = f0.repeat_interleave(cfg.total_upsample, dim=1)[:, None]
    ph, nz = oh.draw_source_randoms(cfg, 1, S, seed=5)
    nz = torch.zeros_like(nz)
    s32, _ = oh.sine_gen(cfg, f0_up, ph, nz, scan_dtype=torch.float32)
    s64, _ = oh.sine_gen(cfg, f0_up, ph, nz, scan_dtype=torch.float64)
    d = (s32 - s64).abs().max().item()
    bound, c_max = H.scan_drift_bound(cfg, f0_up)
    msg = f"T={T} seed={seed}: L-inf {d:.3e}, bound {bound:.3e}, C_max {c_max:.1f}"
    print(msg)
    assert d <= bound, msg
    if T == 500:
        assert d > 0, "the fp32 and fp64 scans are different quantities"
