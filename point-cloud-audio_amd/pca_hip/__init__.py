"""pca_hip: MI355X (gfx950) kernels for the point-cloud-audio hot path, bound over the C ABI
of libpca_hip.so (include/pca_hip.h)."""
from ._lib import LIB_PATH, PcaHipError, lib  # noqa: F401
from .ops import (MAXK, NORM_NFFT, NORM_WIN, RANDK, Deltas, FilterBank, FrameLevel, Pcen, clip_aggregate, clip_rms, cross_entropy, eval_metrics, eval_tally, frame_points, frame_points_bands, frame_points_delta, frame_points_ex, frame_points_masked, frame_points_multires, frame_points_pcen, frame_points_reassigned, get_mode, importance_kernel,  # noqa: F401
                  importance_points, linear, mab, mab_infer, mel_bank, pack_points_2d, pack_points_2d_seq, pack_points_2d_ss, pack_points_3d,
                  pack_points_3d_seq, peak_points, pma_attention, resample, select_points, set_mode, stft_logmag, stft_logmag_batch,
                  subsample_points, trim, trim_batch)
from .baseline import SEL_ALL, BaselineEngine, baseline_config  # noqa: F401
