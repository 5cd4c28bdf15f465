"""tempestsdr.jl_amd -- MI355X-native IQ -> frame reconstruction behind TempestSDR.jl's API.

The directory name carries a dot, so it cannot be imported with a plain `import`; use

    from tempest_loader import load_package      # repo root
    tsdr = load_package()                        # registers it as `tempestsdr_jl_amd`

Contents: csrc/ (hand-written HIP kernels + the C ABI), _lib.py (ctypes binding),
api.py (host mirror with the reference's function names), hires.py (frame averaging at the
monitor's own resolution), register.py (its registration to the raster pixel), display.py (ROI crop, range stretch and 8-bit output of any picture), synth.py (synthetic leak
generator for tests/bench), video_configurations.py and dat_files.py (the callers'
data formats either side of the hot path), parallel.py (one-process-per-GPU sharding),
julia/TempestHIP.jl (the `ccall` shim the Julia runtime loads).
"""
from . import _lib  # noqa: F401
from ._lib import RENDER_H, RENDER_W, TempestHIPError  # noqa: F401
from .api import (Context, Group, Resampler, StagingRing, SyncXY, amDemod, calculate_autocorrelation, default_context,  # noqa: F401
                  downgradeImage, fmDemod, getSpectrum, getWaterfall, getWelch, init_resampler, invert_amDemod,
                  naiveResampler, sig_to_image, vsync, zoom_autocorr)
from .display import display_u8, display_u8_d  # noqa: F401
from .fold import fold, fold_d, fold_plan, fold_scan, fold_scan_d, refine_period  # noqa: F401
from .cfold import cfold, cfold_d, cfold_scan, cfold_scan_d, refine_carrier  # noqa: F401
from .cstack import cstack, cstack_d, cstack_plan  # noqa: F401
from .ctrack import (constant_track, ctrack_probe, ctrack_probe_d, ctrack_stack, ctrack_stack_d, fit_track,  # noqa: F401
                     refine_track)
from .gram import (blind_track, coherent_period_scan, ctrack_gram, ctrack_gram_d, gram_carrier, gram_energy, gram_phases,  # noqa: F401
                   gram_track, track_slopes)
from .tune import Tuner, design_lowpass, freq_fix, phase_fix, tune, tune_d, tune_plan, tune_tile, tuned_t0  # noqa: F401
