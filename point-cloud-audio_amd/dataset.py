"""Point-cloud datasets on MI355X: drop-in for the set-model datasets of ``Code/dataset.py``.

``ESC_pc`` (Code/dataset.py:30-54) and ``ESC_pc_temp`` (Code/dataset.py:138-166) keep their
constructor signatures, ``__len__`` and ``__getitem__`` -> ``(points float32, label int64)``
contract, so ``torch.utils.data.DataLoader(ESC_pc(x, y, farr), ...)`` written against the
reference still runs.  What changes is where the work happens: the log-magnitude
spectrogram is uploaded once and stays resident in HBM; a whole batch of point sets is
assembled by ONE kernel launch (``batch(idx)``), instead of one numpy concatenate per
item on the host (45.6 us / 331 us per set in the reference).  ``__getitem__`` is the same
kernel with a batch of one, copied back to the host because that is what its contract
returns.  ``DeviceBatchLoader`` is the loader the train / eval entry points use.
"""
from typing import Iterator, Optional, Tuple

import copy
import math

import numpy as np
import torch
from torch.utils.data import Dataset

import pca_hip

__all__ = ["ESC_baseline", "ESC_pc", "ESC_pc_ss", "ESC_baseline_temporal",
           "ESC_baseline_temporal_maxK", "ESC_pc_temp", "ESC_pc_temp_maxKSS",
           "ESC_pc_temp_randKSS", "ESC_pc_temp_importancerandKSS", "ESC_wave_pc",
           "ESC_wave_pc_temp", "ESC_wave_pc_multires", "multires_layout", "wave_span_offsets",
           "PeakPoints", "DeviceBatchLoader"]


def _dev(device) -> torch.device:
    return torch.device("cuda", torch.cuda.current_device()) if device is None \
        else torch.device(device)


# ---- datasets of the two comparison baselines (FB, CNN_temp) -------------------------------
# Not point sets and not on the accelerated path: host
# numpy, exactly the item contract of the reference, so that Code/baseline_eval.py and
# Code/baseline_temp_eval.py keep importing them from here.  NOTE the return order: these
# three yield (label, x); the point-cloud datasets yield (points, label).

class ESC_baseline(Dataset):
    """FB items (Code/dataset.py:10-27): x [N, T] spectral frames, y int[T].
    Item idx -> (y[idx], tensor(x[:, idx]))."""

    def __init__(self, x, y):
        self.x = x
        self.labels = y

    def __len__(self):
        return self.x.shape[1]

    def __getitem__(self, idx):
        return self.labels[idx], torch.tensor(self.x[:, idx])


class ESC_baseline_temporal(Dataset):
    """CNN_temp items (Code/dataset.py:82-99): x [N, Nt, T] chunked spectrograms, y int[T].
    Item idx -> (tensor(y[idx]), tensor(x[:, :, idx]).T) i.e. [Nt, N]."""

    def __init__(self, x, y):
        self.x = x
        self.labels = y

    def __len__(self):
        return self.x.shape[2]

    def __getitem__(self, idx):
        return torch.tensor(self.labels[idx]), torch.tensor(self.x[:, :, idx]).T


class ESC_baseline_temporal_maxK(Dataset):
    """CNN_temp items with all but K cells of the chunk zeroed (Code/dataset.py:101-135).
    flag "max": keep the K largest values (``(-v).argsort()[:K]`` over the cells in
    time-major order, as the reference enumerates them); "rand": keep K cells of
    ``np.random.permutation`` (global numpy RNG, as the reference)."""

    def __init__(self, x, y, K, flag="max"):
        self.x = x
        self.labels = y
        self.K = K
        self.flag = flag

    def __len__(self):
        return self.x.shape[2]

    def __getitem__(self, idx):
        xt = self.x[:, :, idx]                        # [N, Nt]
        flat = xt.T.reshape(-1)                        # cell p = t*N + f
        if self.flag == "rand":
            keep = np.random.permutation(flat.shape[0])[:self.K]
        else:
            keep = (-flat).argsort()[:self.K]
        out = np.zeros_like(flat)
        out[keep] = flat[keep]
        return torch.tensor(self.labels[idx]), torch.tensor(out.reshape(xt.shape[1], xt.shape[0]))


class ESC_pc(Dataset):
    """2-D (framewise) point sets: item idx = [(farr[f], x[f, idx]) for f], float32 [F, 2].

    x     array [F, T] log-magnitude spectrogram (numpy or torch, host or device)
    y     int   [T]    label of each frame
    farr  array [F]    normalised frequency of each bin (float64 in the reference, rounded
                       to float32 once here exactly as its ``.float()`` does)
    """

    def __init__(self, x, y, farr, device=None):
        self.x = x
        self.labels = y
        self.farr = farr
        self._device = device
        self._res = None

    @classmethod
    def from_device(cls, spec_tf: torch.Tensor, labels: torch.Tensor, farr) -> "ESC_pc":
        """Wrap a frame-major device spectrogram [T, F] (as ``pca_hip.stft_logmag(...,
        frame_major=True)`` writes it) without a host round trip."""
        self = cls(spec_tf.t(), labels, farr, device=spec_tf.device)
        f32 = torch.as_tensor(np.asarray(farr, dtype=np.float64)).float().to(spec_tf.device)
        self._res = (spec_tf.contiguous(), f32, labels.to(spec_tf.device, torch.int64))
        return self

    def __len__(self):
        return self.x.shape[1]

    def _resident(self):
        if self._res is None:
            dev = _dev(self._device)
            x = torch.as_tensor(self.x).to(dev, torch.float32)
            spec_tf = x.t().contiguous()                      # [T, F]: one set = one row
            f32 = torch.as_tensor(np.asarray(self.farr, dtype=np.float64)).float().to(dev)
            lab = torch.as_tensor(np.asarray(self.labels)).to(dev, torch.int64)
            self._res = (spec_tf, f32, lab)
        return self._res

    @property
    def num_points(self) -> int:
        return int(self.x.shape[0])

    def batch(self, idx: torch.Tensor, out=None, labels_out=None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
        """idx int64[B] on the device -> (points [B, F, 2] float32, labels int64[B])."""
        spec_tf, f32, lab = self._resident()
        return pca_hip.pack_points_2d(spec_tf, f32, idx, lab, frame_major=True, out=out,
                                      labels_out=labels_out)

    def batch_seq(self, idx_seq, step_dev, base_dev, B: int, out=None, labels_out=None):
        """Batch number ``step_dev[0] - base_dev[0]`` of a pre-staged index sequence (the
        Trainer's device cursor: no per-step index upload)."""
        spec_tf, f32, lab = self._resident()
        return pca_hip.pack_points_2d_seq(spec_tf, f32, idx_seq, step_dev, base_dev, B, lab,
                                          frame_major=True, out=out, labels_out=labels_out)

    def __getitem__(self, idx):
        spec_tf, _, _ = self._resident()
        i = torch.tensor([int(idx)], dtype=torch.int64, device=spec_tf.device)
        pts, lbl = self.batch(i)
        return pts[0].cpu(), lbl[0].cpu()


class ESC_pc_temp(Dataset):
    """3-D (spectro-temporal) point sets: item idx = all (f, t) pairs of chunk idx,
    float32 [Nt*F, 3] with columns (farr[f], tarr[t], x[f, t, idx]) and point order
    p = t*F + f (Code/dataset.py:160-166).

    x [F, Nt, S], y int[S], farr [F], tarr [Nt].

    ``nt_valid`` (optional int[S], extension): chunk s holds only nt_valid[s] <= Nt frames (the
    reference discards such short chunks, Code/settransformertemp.py:54-58).  ``batch`` then
    returns padded sets and a third value, the int32 point count of every set, which
    ``ST.forward(X, lengths)`` / the engine take to ignore the padding.
    """

    def __init__(self, x, y, farr, tarr, device=None, nt_valid=None):
        self.x = x
        self.labels = y
        self.farr = farr
        self.tarr = tarr
        self._device = device
        self._res = None
        self.nt_valid = nt_valid
        self._ntv = None

    @property
    def variable_length(self) -> bool:
        return self.nt_valid is not None

    @classmethod
    def from_device(cls, spec_stf: torch.Tensor, labels: torch.Tensor, farr, tarr
                    ) -> "ESC_pc_temp":
        """Wrap a chunk-major device tensor [S, Nt, F] (one set contiguous)."""
        self = cls(spec_stf.permute(2, 1, 0), labels, farr, tarr, device=spec_stf.device)
        dev = spec_stf.device
        self._res = (spec_stf.contiguous().permute(2, 1, 0),
                     torch.as_tensor(np.asarray(farr, dtype=np.float64)).float().to(dev),
                     torch.as_tensor(np.asarray(tarr, dtype=np.float64)).float().to(dev),
                     labels.to(dev, torch.int64))
        return self

    def __len__(self):
        return self.labels.shape[0]

    @property
    def num_points(self) -> int:
        return int(self.x.shape[0] * self.x.shape[1])

    def _resident(self):
        if self._res is None:
            dev = _dev(self._device)
            x = torch.as_tensor(self.x).to(dev, torch.float32)          # [F, Nt, S]
            stf = x.permute(2, 1, 0).contiguous()                        # [S, Nt, F]
            self._res = (stf.permute(2, 1, 0),                           # view [F, Nt, S]
                         torch.as_tensor(np.asarray(self.farr, dtype=np.float64)).float().to(dev),
                         torch.as_tensor(np.asarray(self.tarr, dtype=np.float64)).float().to(dev),
                         torch.as_tensor(np.asarray(self.labels)).to(dev, torch.int64))
        return self._res

    def batch(self, idx: torch.Tensor, out=None, labels_out=None, lengths_out=None):
        spec, f32, t32, lab = self._resident()
        if self.nt_valid is None:
            return pca_hip.pack_points_3d(spec, f32, t32, idx, lab, out=out,
                                          labels_out=labels_out)
        if self._ntv is None:
            self._ntv = torch.as_tensor(np.asarray(self.nt_valid)).to(spec.device, torch.int32)
        return pca_hip.pack_points_3d(spec, f32, t32, idx, lab, out=out, labels_out=labels_out,
                                      nt_valid=self._ntv, lengths_out=lengths_out)

    def batch_seq(self, idx_seq, step_dev, base_dev, B: int, out=None, labels_out=None,
                  lengths_out=None):
        """Batch number ``step_dev[0] - base_dev[0]`` of a pre-staged index sequence."""
        spec, f32, t32, lab = self._resident()
        ntv = None
        if self.nt_valid is not None:
            if self._ntv is None:
                self._ntv = torch.as_tensor(np.asarray(self.nt_valid)).to(spec.device,
                                                                          torch.int32)
            ntv = self._ntv
        return pca_hip.pack_points_3d_seq(spec, f32, t32, idx_seq, step_dev, base_dev, B, lab,
                                          out=out, labels_out=labels_out, nt_valid=ntv,
                                          lengths_out=lengths_out)

    def __getitem__(self, idx):
        spec = self._resident()[0]
        i = torch.tensor([int(idx)], dtype=torch.int64, device=spec.device)
        res = self.batch(i)
        pts, lbl = res[0], res[1]
        if self.nt_valid is not None:            # the un-padded set
            return pts[0, :int(res[2][0])].cpu(), lbl[0].cpu()
        return pts[0].cpu(), lbl[0].cpu()


class ESC_pc_ss(Dataset):
    """2-D point sets of the sub-sampling experiments (Code/dataset.py:58-80): ``x`` and
    ``farr`` are the [K, T] outputs of ``utils.pc_maxK`` / ``pc_randK`` (per-frame values and
    per-frame frequency coordinates); item idx = stack(farr[:, idx], x[:, idx]).T float32."""

    def __init__(self, x, y, farr, device=None):
        self.x = x
        self.labels = y
        self.farr = farr
        self._device = device
        self._res = None

    def __len__(self):
        return self.x.shape[1]

    @property
    def num_points(self) -> int:
        return int(self.x.shape[0])

    def _resident(self):
        if self._res is None:
            dev = _dev(self._device)
            x_tk = torch.as_tensor(np.asarray(self.x)).to(dev, torch.float32).t().contiguous()
            f_tk = torch.as_tensor(np.asarray(self.farr)).to(dev, torch.float32).t().contiguous()
            lab = torch.as_tensor(np.asarray(self.labels)).to(dev, torch.int64)
            self._res = (x_tk, f_tk, lab)
        return self._res

    def batch(self, idx: torch.Tensor, out=None, labels_out=None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
        x_tk, f_tk, lab = self._resident()
        return pca_hip.pack_points_2d_ss(x_tk, f_tk, idx, lab, out=out, labels_out=labels_out)

    def __getitem__(self, idx):
        x_tk = self._resident()[0]
        i = torch.tensor([int(idx)], dtype=torch.int64, device=x_tk.device)
        pts, lbl = self.batch(i)
        return pts[0].cpu(), lbl[0].cpu()


class _TempSS(ESC_pc_temp):
    """3-D point sets reduced to K points per set on the device (one launch per batch)."""
    _mode = pca_hip.MAXK

    def __init__(self, x, y, farr, tarr, K, device=None, seed: int = 0):
        super().__init__(x, y, farr, tarr, device=device)      # dense chunks only
        self.K = int(K)
        self.seed = int(seed)
        self._draw = 0

    @property
    def num_points(self) -> int:
        return self.K

    batch_seq = None        # selections are drawn per call: the Trainer uploads indices per step

    @property
    def stochastic(self) -> bool:
        """True when every call must draw a NEW selection (random-K, multinomial importance
        sampling): a caller that captures ``batch`` into a hipGraph then has to pass
        ``draw_dev`` - a device counter it advances per replay - because the host-side draw
        number is a by-value kernel argument and would be frozen in the captured launch."""
        return self._mode == pca_hip.RANDK

    def batch(self, idx: torch.Tensor, out=None, labels_out=None, want_sel: bool = False,
              draw_dev=None):
        spec, f32, t32, lab = self._resident()
        self._draw += 1
        return pca_hip.subsample_points(spec, f32, t32, idx, self.K, self._mode, self.seed,
                                        self._draw, lab, out=out, labels_out=labels_out,
                                        want_sel=want_sel, draw_dev=draw_dev)

    def __getitem__(self, idx):
        """float64 [K, 3] exactly as the reference builds it (float64 farr / tarr, the float32
        spectrogram widened): the device picks the points, the host gathers the rows."""
        spec = self._resident()[0]
        i = torch.tensor([int(idx)], dtype=torch.int64, device=spec.device)
        _, lbl, sel = self.batch(i, want_sel=True)
        p = sel[0].cpu().numpy().astype(np.int64)
        F = int(spec.shape[0])
        f, t = p % F, p // F
        farr = np.asarray(self.farr, dtype=np.float64)
        tarr = np.asarray(self.tarr, dtype=np.float64)
        v = spec[:, :, int(idx)].cpu().numpy().astype(np.float64)[f, t]
        pc = np.stack((farr[f], tarr[t], v), axis=1)
        return torch.tensor(pc), lbl[0].cpu()


class ESC_pc_temp_maxKSS(_TempSS):
    """The K largest-magnitude points of chunk idx in descending order (Code/dataset.py:169-199:
    ``(-pc[:, -1]).argsort()[:K]``); equal values keep ascending point order."""
    _mode = pca_hip.MAXK


class ESC_pc_temp_randKSS(_TempSS):
    """K points of a uniformly random permutation of chunk idx (Code/dataset.py:201-239).  The
    reference draws from the global numpy RNG; here every draw comes from the counter-based
    device stream (seed, draw number, set), so runs are reproducible per ``seed`` and only
    the distribution matches the reference."""
    _mode = pca_hip.RANDK


class ESC_pc_temp_importancerandKSS(_TempSS):
    """Importance-sampled 3-D point sets (Code/dataset.py:243-289, the rebuttal experiment):
    a heat map (spectrogram gradient magnitude smoothed by a 2 x winF Kaiser kernel, + 1e-6)
    picks K points per chunk: ``choice`` 0 = K draws with replacement from the normalised
    heat map, 1 = the K hottest cells.  The selected flat heat index addresses the
    time-major point table exactly as in the reference (see pca_importance_points).
    Random draws come from the counter-based device stream (``seed``), not torch's global
    generator."""

    def __init__(self, x, y, farr, tarr, K, choice, winF, device=None, seed: int = 0):
        super().__init__(x, y, farr, tarr, K, device=device, seed=seed)
        self.choice = int(choice)
        self.winF = int(winF)
        self._kern = None

    @property
    def stochastic(self) -> bool:
        return self.choice == 0

    def batch(self, idx: torch.Tensor, out=None, labels_out=None, want_sel: bool = False,
              want_heat: bool = False, draw_dev=None):
        spec, f32, t32, lab = self._resident()
        if self._kern is None:
            self._kern = pca_hip.importance_kernel(self.winF).to(spec.device)
        self._draw += 1
        return pca_hip.importance_points(spec, f32, t32, idx, self.K, self.choice, self._kern,
                                         self.seed, self._draw, lab, out=out,
                                         labels_out=labels_out, want_sel=want_sel,
                                         want_heat=want_heat, draw_dev=draw_dev)


def wave_set_offsets(lengths, hop: int, ntemp: int = 1) -> list:
    """Prefix sum of the sets each clip yields: 1 + L // hop frames (librosa's center=True count),
    or, with ntemp > 1, frames // ntemp whole chunks - the short tail is dropped, as
    Code/settransformertemp.py:54-58 does."""
    off = [0]
    for n in lengths:
        off.append(off[-1] + (1 + int(n) // hop) // ntemp)
    return off


class ESC_wave_pc(Dataset):
    """2-D point sets framed from the resident WAVEFORMS per batch: what the pre-pass
    Code/settransformer.py:43-53 plus ``ESC_pc`` give, without the spectrogram - and therefore free to
    move the frame.  Item idx = frame idx of the corpus (clip after clip, 1 + L // hop frames each),
    float32 [F, 2] rows (farr[f], log(1e-8 + |stft| / norm)) from ONE launch per batch
    (pca_frame_points), with per batch slot

    jitter       a time shift of up to +-jitter samples (the centre stays inside the clip)
    gain_db      a level change of up to +-gain_db dB
    win_lengths  a window length drawn out of this sequence (each in [1, n_fft]; None: n_fft).  The first
                 entry is the nominal one: what ``plain()`` uses
    speeds       a playback speed drawn out of this sequence (up to 8, each in [0.5, 2.0]; None: 1.0): the
                 clip resampled by 1 / speed (``pca_hip.resample``'s filter) while the frame is cut, which
                 moves its content along the frequency axis.  The first entry is the nominal one;
                 ``plain()`` uses 1.0
    mix_clips    background waveforms (a list, or "self": the dataset's own clips), one of which is added
                 with probability ``mix_prob``, read circularly from a random start, at a signal-to-noise
                 ratio (clip RMS over background RMS) uniform in ``mix_snr_db`` = (lo, hi) dB.  Labels
                 stay those of the clip
    mix_targets  True: the mix is between-class learning / mixup - ``batch`` also fills the soft target
                 of every slot (``labels2_out`` = the class of the background clip, ``weight_out`` = the
                 weight 1 / (1 + 10^(-snr/20)) of the slot's own label: the clip's share of the amplitude
                 after RMS matching, about 0.09 .. 0.91 for ``mix_snr_db=(-20, 20)``; a slot that does not
                 mix carries its own label twice at weight 1), for ``pca_hip.cross_entropy`` /
                 ``STEngine.fwd_bwd`` / the ``Trainer``.  Needs ``mix_clips``, and with a list of clips
                 ``mix_labels``, one class per background clip ("self": the clip labels)
    freq_masks / freq_mask_width   SpecAugment's frequency masking on the point set: ``freq_masks`` (0 .. 4)
                 bands per set, each 0 .. ``freq_mask_width`` bins wide at a uniform position, are removed;
                 ``freq_masks * freq_mask_width < F``
    time_masks / time_mask_width   likewise stripes of whole frames of a chunk (``ESC_wave_pc_temp``;
                 ``time_masks * time_mask_width < Ntemp``)
    mask_mode    "drop": the masked points are absent - ``batch`` compacts the kept points to the front of
                 every set, zero-fills behind them and appends ``lengths`` (int32 [B], the point counts) to
                 what it returns; the dataset is then ``variable_length`` and the ``Trainer`` hands the
                 counts to the step.  "floor": the sets stay dense, a masked point keeps its coordinates
                 and carries a silent bin's value log(1e-8) - for runs that want the dense step (at d = 128
                 the set-resident forward takes no ``lengths``).  ``plain()`` switches the masks off

    drawn from the counter-based device stream (seed, draw number, batch slot, set), as
    ``ESC_pc_temp_randKSS`` draws its points.  With all three off the batches are bit for bit those of
    ``ESC_pc`` over ``pca_hip.stft_logmag_batch`` of the same clips.  With speeds and mix off a batch is
    one pca_frame_points launch; with either on, one pca_frame_points_ex launch; with a mask on, one
    pca_frame_points_masked launch (the same kernel).

    clips  list of 1-D float32 waveforms (numpy or torch, host or device), each longer than n_fft / 2
    y      one label per clip
    norm   "n_fft": magnitude / n_fft (the train scripts); "win": / the window length (Code/pceval.py:76)
    reassign  None: the grid rows above.  True, or a dict of ``axes``, ``rel_floor``, ``abs_floor``,
           ``max_df``, ``max_dt``, ``strength`` (``pca_hip.frame_points_reassigned``): every bin that carries
           energy is written at its instantaneous frequency (and, 3-D, group delay) instead of its grid
           coordinates, with the same value - one pca_frame_points_reassigned launch per batch.  Defaults:
           axes "f" for 2-D sets and "ft" for 3-D sets (Ntemp >= 2), rel_floor log(1e3), abs_floor -inf,
           max_df 2 bins, max_dt 1 frame, strength 1.  A representation, not an augmentation: ``plain()``
           keeps it, ``stochastic`` ignores it, the sets stay dense.  It composes with jitter, gain_db,
           win_lengths and norm; with speeds, the mix or the masks it raises ``ValueError`` (those live in
           pca_frame_points_ex: out of scope).  ``with_reassign(spec_or_None)`` gives a view on the same
           resident waveforms with another setting
    bands  None: one point per FFT bin, as above.  A ``pca_hip.FilterBank`` over this n_fft
           (``pca_hip.mel_bank(fs, n_fft, n_mels)`` for log-mel): one point per band,
           (centres[m] / fs, [t,] log(amin + sum_k W[m, k] |stft|^power)), the bins summed inside the frame
           launch - one pca_frame_points_bands launch per batch.  ``F`` becomes ``n_bands``, ``farr`` the
           bands' centres / fs, ``num_points`` follows.  No reference counterpart.  A representation, not an
           augmentation: ``plain()`` keeps it, ``stochastic`` ignores it, the sets stay dense.  It composes
           with jitter, gain_db, win_lengths and norm; with speeds, the mix, the masks, ``reassign`` or
           ``drop_nyquist=True`` it raises ``ValueError`` (those live in other launches, or cut the bins the
           bank is defined over: out of scope).  ``with_bands(bank_or_None)`` gives a view on the same
           resident waveforms with another bank (None: the grid dataset, bit for bit)
    pcen   None: the band value above, log(amin + E).  A ``pca_hip.Pcen`` (needs ``bands``): per-channel energy
           normalisation in its place - each band's energy divided by a smoothed version of itself over
           ``pcen.context`` frames before the set and the set's own, then a root (``librosa.pcen``'s formula,
           parity by formula and unpinned) - one pca_frame_points_pcen launch per batch.  The smoother's
           coefficient follows from ``pcen.time_constant``, ``fs`` and ``hop``.  Shapes, axes, labels, meta and
           the draws are those of the band dataset.  A representation like ``bands``: ``plain()`` keeps it,
           ``with_pcen(None)`` is the band dataset bit for bit, the refusals of ``bands`` carry over, and
           ``pcen`` without ``bands`` raises ``ValueError``
    deltas None: rows (f, [t,] value).  A ``pca_hip.Deltas(axes, width)``: regression deltas of the value column
           ride along as further point columns - dt, how the value moves over ``width`` frames before and after
           (the context frames are cut from the clip around the set; outside the clip its end frames repeat),
           and / or df, how it moves over ``width`` rows below and above (edge rows replicated) - rows
           (f, [t,] value, deltas in the order of ``axes``), one pca_frame_points_delta launch per batch.
           ``din`` becomes 2 or 3 plus the number of axes and is at most 4: a 3-D set takes one axis, a 2-D set
           one or two.  ``F``, ``farr``, ``num_points``, labels, meta and the draws are those of the underlying
           grid or band dataset.  A representation: ``plain()`` keeps it, ``stochastic`` ignores it,
           ``with_deltas(None)`` is the underlying dataset bit for bit.  It composes with jitter, gain_db,
           win_lengths, norm, ``drop_nyquist`` and ``bands``; with speeds, the mix, ``mix_targets``, the masks,
           ``reassign`` or ``pcen`` it raises ``ValueError`` (out of scope), and ``PeakPoints`` refuses it
    """
    _ntemp = 1

    def __init__(self, clips, y, fs, n_fft, hop=None, drop_nyquist=False, jitter=0, gain_db=0.0,
                 win_lengths=None, norm="n_fft", seed=0, device=None, speeds=None, mix_clips=None,
                 mix_prob=0.0, mix_snr_db=(0.0, 20.0), mix_targets=False, mix_labels=None,
                 freq_masks=0, freq_mask_width=0, time_masks=0, time_mask_width=0, mask_mode="drop",
                 reassign=None, bands=None, pcen=None, deltas=None):
        self._setup(clips, y, fs, n_fft, hop, drop_nyquist, jitter, gain_db, win_lengths, norm, seed,
                    device)
        self._setup_ex(speeds, mix_clips, mix_prob, mix_snr_db, mix_targets, mix_labels)
        self._setup_mask(freq_masks, freq_mask_width, time_masks, time_mask_width, mask_mode)
        self._setup_reassign(reassign)
        self._setup_bands(bands)
        self._setup_pcen(pcen)
        self._setup_deltas(deltas)

    def _setup(self, clips, y, fs, n_fft, hop, drop_nyquist, jitter, gain_db, win_lengths, norm, seed,
               device):
        if norm not in ("n_fft", "win"):
            raise ValueError(f"norm is 'n_fft' or 'win', got {norm!r}")
        self.clips, self.clip_labels = list(clips), np.asarray(y).astype(np.int64)
        assert len(self.clips) == len(self.clip_labels) > 0
        self.fs, self.n_fft = fs, int(n_fft)
        self.hop = self.n_fft // 2 if hop is None else int(hop)
        self.F = self.n_fft // 2 if drop_nyquist else self.n_fft // 2 + 1
        self.farr = np.linspace(0, fs / 2, self.F) / fs
        self._grid = (self.F, self.farr, bool(drop_nyquist))   # what with_bands(None) puts back
        self.bands = None
        self.pcen = None
        self.deltas = None
        self.tarr = None
        self.jitter, self.gain_db = int(jitter), float(gain_db)
        self.win_lengths = (self.n_fft,) if win_lengths is None else tuple(int(w) for w in win_lengths)
        if not self.win_lengths or not all(1 <= w <= self.n_fft for w in self.win_lengths):
            raise ValueError(f"win_lengths {self.win_lengths}: each in [1, n_fft = {self.n_fft}]")
        self.norm = norm
        self.seed = int(seed)
        self._draw = 0
        self._device = device
        self._store = {}                  # the resident tensors, shared with plain() views
        self.lengths = [int(c.shape[0]) for c in self.clips]
        self._max_len, self._min_len = max(self.lengths), min(self.lengths)
        self.wave_off = [0] + list(np.cumsum(self.lengths))
        self.set_off = wave_set_offsets(self.lengths, self.hop, self._ntemp)
        # label of every set (what ESC_pc calls labels)
        self.labels = np.repeat(self.clip_labels, np.diff(self.set_off))

    def _setup_ex(self, speeds, mix_clips, mix_prob, mix_snr_db, mix_targets=False, mix_labels=None):
        """Speed change and background mix: checked here, on the host, like win_lengths."""
        self.speeds = (1.0,) if speeds is None else tuple(float(v) for v in speeds)
        if not 1 <= len(self.speeds) <= 8 or not all(0.5 <= v <= 2.0 for v in self.speeds):
            raise ValueError(f"speeds {self.speeds}: 1 to 8 values, each in [0.5, 2.0]")
        self.ratios = tuple(1.0 / v for v in self.speeds)
        self.mix_prob = float(mix_prob)
        if not 0.0 <= self.mix_prob <= 1.0:
            raise ValueError(f"mix_prob {mix_prob} outside [0, 1]")
        lo, hi = (float(v) for v in mix_snr_db)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
            raise ValueError(f"mix_snr_db {mix_snr_db}: finite (lo, hi) with lo <= hi")
        self.mix_snr_db = (lo, hi)
        if self.mix_prob > 0.0 and mix_clips is None:
            raise ValueError("mix_prob > 0 needs mix_clips (a list of waveforms, or 'self')")
        if isinstance(mix_clips, str) and mix_clips != "self":
            raise ValueError(f"mix_clips is a list of waveforms or 'self', got {mix_clips!r}")
        self.mix_clips = mix_clips if mix_clips is None or isinstance(mix_clips, str) else list(mix_clips)
        if isinstance(self.mix_clips, list) and (
                not self.mix_clips or any(int(c.shape[0]) < 1 for c in self.mix_clips)):
            raise ValueError("mix_clips: at least one waveform, none of them empty")
        self.mix_targets = bool(mix_targets)
        self.mix_labels = None
        if self.mix_targets:
            if self.mix_clips is None:
                raise ValueError("mix_targets needs mix_clips (a list of waveforms, or 'self')")
            if isinstance(self.mix_clips, list):
                if mix_labels is None:
                    raise ValueError("mix_targets with a list of mix_clips needs mix_labels "
                                     "(one class per background clip)")
                self.mix_labels = np.asarray(mix_labels).astype(np.int64).reshape(-1)
                if len(self.mix_labels) != len(self.mix_clips):
                    raise ValueError(f"mix_labels: {len(self.mix_labels)} labels for "
                                     f"{len(self.mix_clips)} mix_clips")
        if self._speed_on and int(self._min_len * min(self.ratios)) <= self.n_fft // 2:
            raise ValueError(f"speeds {self.speeds}: the shortest clip ({self._min_len} samples) at speed "
                             f"{max(self.speeds)} is no longer than n_fft / 2 = {self.n_fft // 2}")

    def _setup_mask(self, freq_masks, freq_mask_width, time_masks, time_mask_width, mask_mode):
        """Frequency bands and time stripes of points to remove: checked here, on the host, by the rules
        of pca_frame_points_masked."""
        pca_hip.ops.point_mask(self.F, self._ntemp, freq_masks, freq_mask_width, time_masks,
                               time_mask_width, mask_mode)
        self.freq_masks, self.freq_mask_width = int(freq_masks), int(freq_mask_width)
        self.time_masks, self.time_mask_width = int(time_masks), int(time_mask_width)
        self.mask_mode = mask_mode

    def _setup_reassign(self, reassign):
        """``reassign``: None, True or a dict of the fields of pca_frame_points_reassigned's spec; checked
        here, on the host, by that launch's rules."""
        self.reassign = None
        if reassign is None or reassign is False:
            return
        spec = dict(axes="ft" if self.tarr is not None and self._ntemp >= 2 else "f",
                    rel_floor=math.log(1e3), abs_floor=float("-inf"), max_df=2.0, max_dt=1.0, strength=1.0)
        if reassign is not True:
            unknown = set(reassign) - set(spec)
            if unknown:
                raise ValueError(f"reassign: unknown fields {sorted(unknown)} (known: {sorted(spec)})")
            spec.update(reassign)
        if self._speed_on or self._mix_on or self.mix_targets or self._mask_on:
            raise ValueError("reassign does not combine with speeds, the mix or the masks: those live in "
                             "pca_frame_points_ex, reassignment in pca_frame_points_reassigned")
        c = pca_hip.ops.reassign_spec(**spec)
        if c.axes & 2 and (self.tarr is None or self._ntemp < 2):
            raise ValueError(f"reassign axes {spec['axes']!r}: the time axis needs a 3-D dataset with "
                             f"Ntemp >= 2")
        if self.F < 2:
            raise ValueError("reassign needs at least 2 frequency bins")
        self.reassign = spec

    def with_reassign(self, reassign):
        """A view on the same resident waveforms with another ``reassign`` (None: the grid dataset);
        everything else, the augmentations and the draw counter's value included, is kept."""
        if self.bands is not None and reassign not in (None, False):
            raise ValueError("reassign does not combine with bands: reassignment moves FFT bins, a band "
                             "set has none (pca_frame_points_reassigned / pca_frame_points_bands)")
        if self.deltas is not None and reassign not in (None, False):
            raise ValueError("reassign does not combine with deltas: a delta differences grid neighbours, "
                             "reassigned points have left the grid - out of scope")
        v = copy.copy(self)
        v._setup_reassign(reassign)
        return v

    def _setup_bands(self, bands):
        """``bands``: None or a ``pca_hip.FilterBank`` over this n_fft; checked here, on the host."""
        self.bands = None
        self.F, self.farr = self._grid[0], self._grid[1]
        if bands is None:
            return
        if not isinstance(bands, pca_hip.FilterBank):
            raise TypeError(f"bands is a pca_hip.FilterBank (pca_hip.mel_bank(...)) or None, got "
                            f"{type(bands).__name__}")
        if self._speed_on or self._mix_on or self.mix_targets or self._mask_on or self.reassign is not None:
            raise ValueError("bands do not combine with speeds, the mix, the masks or reassign: those live in "
                             "other launches (pca_frame_points_ex, pca_frame_points_reassigned), the band "
                             "sums in pca_frame_points_bands - out of scope")
        if self._grid[2] and not isinstance(self, ESC_wave_pc_temp):   # the 3-D grid's own drop is not the caller's
            raise ValueError("bands do not combine with drop_nyquist=True: a bank is defined over all "
                             "n_fft/2 + 1 bins (leave the Nyquist bin out of the bank instead) - out of scope")
        if bands.n_src != self.n_fft // 2 + 1:
            raise ValueError(f"bands cover {bands.n_src} bins, n_fft = {self.n_fft} has "
                             f"{self.n_fft // 2 + 1}")
        if self._ntemp * bands.n_bands > 16384:
            raise ValueError(f"bands: {self._ntemp * bands.n_bands} points per set (max 16384)")
        self.bands = bands
        self.F = bands.n_bands
        self.farr = np.asarray(bands.centres, dtype=np.float64) / self.fs

    def with_bands(self, bands):
        """A view on the same resident waveforms with another filter bank (None: the grid dataset, bit for
        bit); everything else, the augmentations and the draw counter's value included, is kept.  ``pcen``
        is kept with a bank and leaves with it."""
        v = copy.copy(self)
        v._setup_bands(bands)
        v._setup_pcen(self.pcen if bands is not None else None)
        return v

    def _setup_pcen(self, pcen):
        """``pcen``: None or a ``pca_hip.Pcen``; checked here, on the host."""
        self.pcen = None
        if pcen is None:
            return
        if not isinstance(pcen, pca_hip.Pcen):
            raise TypeError(f"pcen is a pca_hip.Pcen or None, got {type(pcen).__name__}")
        if self.bands is None:
            raise ValueError("pcen needs bands (a pca_hip.FilterBank): PCEN on grid sets without a bank is out "
                             "of scope")
        self.pcen = pcen

    def with_pcen(self, pcen):
        """A view on the same resident waveforms with another ``pcen`` (None: the band dataset, bit for bit);
        everything else, the bank, the augmentations and the draw counter's value included, is kept."""
        if self.deltas is not None and pcen is not None:
            raise ValueError("pcen does not combine with deltas: each is a ticketed launch of its own "
                             "(pca_frame_points_pcen / pca_frame_points_delta) - out of scope")
        v = copy.copy(self)
        v._setup_pcen(pcen)
        return v

    def _setup_deltas(self, deltas):
        """``deltas``: None or a ``pca_hip.Deltas``; checked here, on the host."""
        self.deltas = None
        if deltas is None:
            return
        if not isinstance(deltas, pca_hip.Deltas):
            raise TypeError(f"deltas is a pca_hip.Deltas or None, got {type(deltas).__name__}")
        if (self._speed_on or self._mix_on or self.mix_targets or self._mask_on or self.reassign is not None
                or self.pcen is not None):
            raise ValueError("deltas do not combine with speeds, the mix, mix_targets, the masks, reassign or "
                             "pcen: those live in other launches (pca_frame_points_ex, "
                             "pca_frame_points_reassigned, pca_frame_points_pcen), the deltas in "
                             "pca_frame_points_delta - out of scope")
        din = (2 if self.tarr is None else 3) + deltas.count
        if din > 4:
            raise ValueError(f"deltas {deltas.axes!r} on a 3-D dataset give din = {din}: a point has at most 4 "
                             f"columns, a 3-D set takes one axis")
        self.deltas = deltas

    def with_deltas(self, deltas):
        """A view on the same resident waveforms with another ``deltas`` (None: the underlying grid or band
        dataset, bit for bit); everything else, the bank, the augmentations and the draw counter's value
        included, is kept."""
        v = copy.copy(self)
        v._setup_deltas(deltas)
        return v

    @property
    def din(self) -> int:
        """Columns of a point: 2 (f, value) or 3 (f, t, value), plus one per delta axis."""
        return (2 if self.tarr is None else 3) + (0 if self.deltas is None else self.deltas.count)

    def _bands_farr(self, dev):
        """The band axis on the device, once per bank, in the store the views share."""
        held = self._store.setdefault("bands_farr", {})
        if id(self.bands) not in held:       # the entry keeps the bank alive, so its id stays its own
            held[id(self.bands)] = (self.bands, torch.as_tensor(self.farr).float().to(dev))
        return held[id(self.bands)][1]

    @property
    def _mask_on(self) -> bool:
        return (self.freq_masks > 0 and self.freq_mask_width > 0) or \
               (self.time_masks > 0 and self.time_mask_width > 0)

    @property
    def variable_length(self) -> bool:
        """True when ``batch`` returns padded sets and their point counts (a mask on in drop mode)."""
        return self._mask_on and self.mask_mode == "drop"

    @property
    def _speed_on(self) -> bool:
        return self.speeds != (1.0,)

    @property
    def _mix_on(self) -> bool:
        return self.mix_prob > 0.0 and self.mix_clips is not None

    @property
    def soft_targets(self) -> bool:
        """True when ``batch`` fills ``labels2_out`` / ``weight_out`` (``mix_targets``): the training
        step then runs on soft targets (``Trainer``)."""
        return self.mix_targets

    def __len__(self):
        return self.set_off[-1]

    @property
    def num_points(self) -> int:
        return self._ntemp * self.F

    batch_seq = None        # augmentations are drawn per call: the Trainer uploads indices per step

    @property
    def stochastic(self) -> bool:
        """True when any augmentation is on: every call must then draw anew, so a caller that
        captures ``batch`` into a hipGraph passes ``draw_dev`` (see ``_TempSS.stochastic``)."""
        return (self.jitter > 0 or self.gain_db > 0.0 or len(self.win_lengths) > 1
                or self._speed_on or self._mix_on or self._mask_on)

    def plain(self, win_length=None):
        """A view on the same resident waveforms with every augmentation off: deterministic, the
        regular frame grid, the nominal window (``win_lengths[0]``, or ``win_length``).  What the
        ``Evaluator`` and ``fit(test_dataset=...)`` take."""
        v = copy.copy(self)
        v.jitter, v.gain_db = 0, 0.0
        v.speeds, v.ratios, v.mix_prob, v.mix_targets = (1.0,), (1.0,), 0.0, False
        v.freq_masks = v.time_masks = 0
        v.win_lengths = (self.win_lengths[0] if win_length is None else int(win_length),)
        if not 1 <= v.win_lengths[0] <= self.n_fft:
            raise ValueError(f"win_length {v.win_lengths[0]} outside [1, n_fft = {self.n_fft}]")
        v._draw = 0
        return v

    def _resident(self):
        if "res" not in self._store:
            dev = _dev(self._device)
            i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dev)   # noqa: E731
            f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).float().to(dev)  # noqa: E731
            waves = torch.cat([torch.as_tensor(c).to(dev, torch.float32).reshape(-1)
                               for c in self.clips])
            self._store["res"] = (waves, i64(self.wave_off), i64(self.set_off), f32(self._grid[1]),
                                  None if self.tarr is None else f32(self.tarr),
                                  i64(self.clip_labels))
            self._store["win"] = {}
            if self._mix_on or self.mix_targets:   # the RMS vectors and the background corpus: once, here
                self._mix_resident()
        return self._store["res"]

    def _win_dev(self, dev):
        if self.win_lengths not in self._store["win"]:
            self._store["win"][self.win_lengths] = torch.tensor(self.win_lengths, dtype=torch.int32,
                                                                 device=dev)
        return self._store["win"][self.win_lengths]

    def _mix_resident(self):
        """The background corpus and both RMS vectors, computed once and kept in the shared store:
        (clip_rms, bg_waves, bg_off, bg_rms, bg_max_len)."""
        if "mix" not in self._store:
            waves, woff = self._resident()[:2]
            rms = pca_hip.clip_rms(waves, woff, self._max_len)
            if self.mix_clips == "self":
                self._store["mix"] = (rms, waves, woff, rms, self._max_len)
            else:
                lens = [int(c.shape[0]) for c in self.mix_clips]
                bg = torch.cat([torch.as_tensor(c).to(waves.device, torch.float32).reshape(-1)
                                for c in self.mix_clips])
                boff = torch.as_tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                                       ).to(waves.device)
                self._store["mix"] = (rms, bg, boff, pca_hip.clip_rms(bg, boff, max(lens)), max(lens))
        return self._store["mix"]

    def _mix_labels_dev(self):
        """The classes of the background clips on the device (``mix_targets``)."""
        if "mix_labels" not in self._store:
            lab = self._resident()[5]
            self._store["mix_labels"] = lab if self.mix_clips == "self" else torch.as_tensor(
                self.mix_labels).to(lab.device)
        return self._store["mix_labels"]

    def batch(self, idx: torch.Tensor, out=None, labels_out=None, draw_dev=None,
              want_meta: bool = False, want_samples: bool = False, labels2_out=None, weight_out=None,
              lengths_out=None):
        """idx int64[B] on the device -> (points [B, num_points, 2 or 3] float32, labels int64[B]
        [, meta int32 [B, 4] = (clip, centre sample of frame 0, window length, bits of the gain)]).
        With ``speeds`` or the mix on, meta is int32 [B, 8] (pca_hip.frame_points_ex: + speed index,
        background clip or -1, its start, bits of its scale) and ``want_samples`` adds the float32
        [B, Ntemp, n_fft] samples of every frame before window and gain.  With ``soft_targets`` the
        return ends with (labels2 int64[B], weight float32[B]), written into ``labels2_out`` /
        ``weight_out`` when given, by the same launch.  With a mask on (pca_hip.frame_points_masked) meta
        is int32 [B, 24] - those 8 columns, then (start, width) of the 4 bands and the 4 stripes - and in
        drop mode the return ends with lengths int32 [B], written into ``lengths_out`` when given."""
        waves, woff, soff, f32, t32, lab = self._resident()
        self._draw += 1
        if self._mask_on:
            mask = dict(freq_masks=self.freq_masks, freq_mask_width=self.freq_mask_width,
                        time_masks=self.time_masks, time_mask_width=self.time_mask_width,
                        mask_mode=self.mask_mode, lengths_out=lengths_out)
        if self._speed_on or self._mix_on or self.mix_targets or self._mask_on:
            mix = {}
            if self._mix_on or self.mix_targets:
                rms, bg, boff, brms, bmax = self._mix_resident()
                mix = dict(clip_rms=rms, bg_waves=bg, bg_off=boff, bg_rms=brms, bg_max_len=bmax,
                           mix_prob=self.mix_prob, mix_snr_db=self.mix_snr_db)
            if self.mix_targets:
                mix.update(bg_labels=self._mix_labels_dev(), labels2_out=labels2_out,
                           weight_out=weight_out)
            launch, mask = (pca_hip.frame_points_masked, mask) if self._mask_on \
                else (pca_hip.frame_points_ex, {})
            return launch(
                waves, woff, soff, idx, self.n_fft, self.hop, self.F, f32, t32, self._ntemp,
                max_len=self._max_len, min_len=self._min_len, clip_labels=lab,
                jitter=self.jitter, gain_db=self.gain_db, win_lengths=self._win_dev(waves.device),
                norm_mode=pca_hip.NORM_WIN if self.norm == "win" else pca_hip.NORM_NFFT,
                seed=self.seed, draw=self._draw, ratios=self.ratios, out=out, labels_out=labels_out,
                draw_dev=draw_dev, want_meta=want_meta, want_samples=want_samples, **mix, **mask)
        if want_samples:
            raise ValueError("want_samples needs speeds or the mix on (pca_hip.frame_points_ex)")
        if self.deltas is not None:
            banded = self.bands is not None
            return pca_hip.frame_points_delta(
                waves, woff, soff, idx, self.n_fft, self.hop, self.F,
                self._bands_farr(waves.device) if banded else f32, t32, self._ntemp, deltas=self.deltas,
                bank=self.bands, max_len=self._max_len, min_len=self._min_len, clip_labels=lab,
                jitter=self.jitter, gain_db=self.gain_db, win_lengths=self._win_dev(waves.device),
                norm_mode=pca_hip.NORM_WIN if self.norm == "win" else pca_hip.NORM_NFFT,
                seed=self.seed, draw=self._draw, out=out, labels_out=labels_out, draw_dev=draw_dev,
                want_meta=want_meta)
        if self.pcen is not None:
            return pca_hip.frame_points_pcen(
                waves, woff, soff, idx, self.n_fft, self.hop, self.bands, self._bands_farr(waves.device), t32,
                self._ntemp, pcen=self.pcen, fs=self.fs, max_len=self._max_len, min_len=self._min_len,
                clip_labels=lab, jitter=self.jitter, gain_db=self.gain_db,
                win_lengths=self._win_dev(waves.device),
                norm_mode=pca_hip.NORM_WIN if self.norm == "win" else pca_hip.NORM_NFFT,
                seed=self.seed, draw=self._draw, out=out, labels_out=labels_out, draw_dev=draw_dev,
                want_meta=want_meta)
        if self.bands is not None:
            return pca_hip.frame_points_bands(
                waves, woff, soff, idx, self.n_fft, self.hop, self.bands, self._bands_farr(waves.device), t32,
                self._ntemp, max_len=self._max_len, min_len=self._min_len, clip_labels=lab,
                jitter=self.jitter, gain_db=self.gain_db, win_lengths=self._win_dev(waves.device),
                norm_mode=pca_hip.NORM_WIN if self.norm == "win" else pca_hip.NORM_NFFT,
                seed=self.seed, draw=self._draw, out=out, labels_out=labels_out, draw_dev=draw_dev,
                want_meta=want_meta)
        if self.reassign is not None:
            return pca_hip.frame_points_reassigned(
                waves, woff, soff, idx, self.n_fft, self.hop, self.F, f32, t32, self._ntemp,
                max_len=self._max_len, min_len=self._min_len, clip_labels=lab,
                jitter=self.jitter, gain_db=self.gain_db, win_lengths=self._win_dev(waves.device),
                norm_mode=pca_hip.NORM_WIN if self.norm == "win" else pca_hip.NORM_NFFT,
                seed=self.seed, draw=self._draw, out=out, labels_out=labels_out, draw_dev=draw_dev,
                want_meta=want_meta, **self.reassign)
        return pca_hip.frame_points(
            waves, woff, soff, idx, self.n_fft, self.hop, self.F, f32, t32, self._ntemp,
            max_len=self._max_len, min_len=self._min_len, clip_labels=lab,
            jitter=self.jitter, gain_db=self.gain_db, win_lengths=self._win_dev(waves.device),
            norm_mode=pca_hip.NORM_WIN if self.norm == "win" else pca_hip.NORM_NFFT,
            seed=self.seed, draw=self._draw, out=out, labels_out=labels_out, draw_dev=draw_dev,
            want_meta=want_meta)

    def __getitem__(self, idx):
        waves = self._resident()[0]
        i = torch.tensor([int(idx)], dtype=torch.int64, device=waves.device)
        res = self.batch(i)
        pts, lbl = res[0], res[1]
        if self.variable_length:                 # the un-padded set
            return pts[0, :int(res[-1][0])].cpu(), lbl[0].cpu()
        return pts[0].cpu(), lbl[0].cpu()


class ESC_wave_pc_temp(ESC_wave_pc):
    """3-D point sets framed from the resident waveforms per batch: the pre-pass
    Code/settransformertemp.py:45-61 plus ``ESC_pc_temp`` without the spectrogram.  Item idx = chunk
    idx of the corpus: ``Ntemp`` consecutive frames of one clip (frames // Ntemp chunks per clip, the
    short tail dropped), float32 [Ntemp * F, 3] rows (farr[f], tarr[t], value), point p = t * F + f,
    the Nyquist bin dropped and tarr = linspace(0, hop / fs * Ntemp, Ntemp) as
    Code/settransformertemp.py:40-41,52.  One shift, gain and window per chunk, so its frames stay
    ``hop`` apart and ``tarr`` keeps its meaning.  Arguments as ``ESC_wave_pc``; with ``bands`` the rows
    are (centres[m] / fs, tarr[t], value), point p = t * n_bands + m, and the bank sees all n_fft/2 + 1
    bins (the grid's dropped Nyquist bin is the grid's affair)."""

    def __init__(self, clips, y, fs, n_fft, Ntemp, hop=None, jitter=0, gain_db=0.0,
                 win_lengths=None, norm="n_fft", seed=0, device=None, speeds=None, mix_clips=None,
                 mix_prob=0.0, mix_snr_db=(0.0, 20.0), mix_targets=False, mix_labels=None,
                 freq_masks=0, freq_mask_width=0, time_masks=0, time_mask_width=0, mask_mode="drop",
                 reassign=None, bands=None, pcen=None, deltas=None):
        self._ntemp = int(Ntemp)
        assert self._ntemp >= 1
        self._setup(clips, y, fs, n_fft, hop, True, jitter, gain_db, win_lengths, norm, seed, device)
        self._setup_ex(speeds, mix_clips, mix_prob, mix_snr_db, mix_targets, mix_labels)
        self._setup_mask(freq_masks, freq_mask_width, time_masks, time_mask_width, mask_mode)
        self.tarr = np.linspace(0, (self.hop / fs) * self._ntemp, self._ntemp)
        self._setup_reassign(reassign)
        self._setup_bands(bands)
        self._setup_pcen(pcen)
        self._setup_deltas(deltas)


def wave_span_offsets(lengths, span: int) -> list:
    """Prefix sum of the sets each clip yields when a set spans ``span`` samples: L // span whole spans,
    the short tail dropped."""
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n) // int(span))
    return off


MULTIRES_MAX_LEVELS, MULTIRES_MAX_POINTS = 4, 16384
_LEVEL_KEYS = ("n_fft", "hop", "Ntemp", "drop_nyquist", "offset", "win_lengths")


def multires_layout(fs, levels, span, time_axis: bool = True) -> dict:
    """Host-side geometry of a multi-resolution point set (``ESC_wave_pc_multires``), checked by the rules
    of pca_frame_points_multires (``ValueError``).

    ``levels``: 1 to 4 dicts of ``n_fft`` (a power of two in [64, 4096]), ``hop`` (default n_fft // 2),
    ``Ntemp`` (frames per set; default span // hop, which must be >= 1), ``drop_nyquist`` (default True),
    ``offset`` (samples from the set's anchor to the centre of the level's frame 0; default 0) and
    ``win_lengths`` (default (n_fft,); each in [1, n_fft], the same count in every level; the first entry is
    the nominal one).  ``span``: samples per set, in (0, 2^30].
    Returns lists with one entry per level - ``n_fft``, ``hop``, ``Ntemp``, ``offset``, ``win_lengths``,
    ``F`` (bins), ``farr`` = linspace(0, fs / 2, F) / fs as ``ESC_wave_pc`` builds it, ``tarr`` (None without
    ``time_axis``, which requires Ntemp == 1 everywhere) and ``point_off`` (the level's first point inside a
    set) - and ``N``, the points per set (at most 16384).
    ``tarr[j] = (offset + j * hop) / fs`` is the TRUE time of frame j in seconds from the set's anchor.  It is
    not the reference's linspace(0, hop / fs * Ntemp, Ntemp) (Code/settransformertemp.py:52), which stretches
    the spacing by Ntemp / (Ntemp - 1) and would put levels of different Ntemp on different clocks."""
    levels = list(levels)
    span = int(span)
    if not 1 <= len(levels) <= MULTIRES_MAX_LEVELS:
        raise ValueError(f"multires: {len(levels)} levels (1 .. {MULTIRES_MAX_LEVELS})")
    if not 0 < span <= 1 << 30:
        raise ValueError(f"multires: span {span} outside (0, 2^30]")
    out = {k: [] for k in ("n_fft", "hop", "Ntemp", "offset", "win_lengths", "F", "farr", "tarr",
                           "point_off")}
    N = 0
    for r, lv in enumerate(levels):
        unknown = set(lv) - set(_LEVEL_KEYS)
        if unknown or "n_fft" not in lv:
            raise ValueError(f"multires level {r}: needs n_fft, knows {_LEVEL_KEYS}, got {sorted(lv)}")
        n_fft = int(lv["n_fft"])
        if not (64 <= n_fft <= 4096 and n_fft & (n_fft - 1) == 0):
            raise ValueError(f"multires level {r}: n_fft {n_fft} must be a power of two in [64, 4096]")
        hop = n_fft // 2 if lv.get("hop") is None else int(lv["hop"])
        if hop < 1:
            raise ValueError(f"multires level {r}: hop {hop}")
        ntemp = span // hop if lv.get("Ntemp") is None else int(lv["Ntemp"])
        if ntemp < 1:
            raise ValueError(f"multires level {r}: Ntemp {ntemp} (span {span}, hop {hop})")
        if not time_axis and ntemp != 1:
            raise ValueError(f"multires level {r}: time_axis=False needs Ntemp == 1, got {ntemp}")
        offset = int(lv.get("offset", 0))
        if abs(offset) > 1 << 30:
            raise ValueError(f"multires level {r}: offset {offset} outside [-2^30, 2^30]")
        wins = (n_fft,) if lv.get("win_lengths") is None else tuple(int(w) for w in lv["win_lengths"])
        if not wins or not all(1 <= w <= n_fft for w in wins):
            raise ValueError(f"multires level {r}: win_lengths {wins}: each in [1, n_fft = {n_fft}]")
        if out["win_lengths"] and len(wins) != len(out["win_lengths"][0]):
            raise ValueError(f"multires level {r}: {len(wins)} win_lengths, level 0 has "
                             f"{len(out['win_lengths'][0])} (one window index serves every level)")
        F = n_fft // 2 if lv.get("drop_nyquist", True) else n_fft // 2 + 1
        for k, v in (("n_fft", n_fft), ("hop", hop), ("Ntemp", ntemp), ("offset", offset),
                     ("win_lengths", wins), ("F", F), ("farr", np.linspace(0, fs / 2, F) / fs),
                     ("tarr", (offset + np.arange(ntemp) * hop) / fs if time_axis else None),
                     ("point_off", N)):
            out[k].append(v)
        N += ntemp * F
    if N > MULTIRES_MAX_POINTS:
        raise ValueError(f"multires: {N} points per set (max {MULTIRES_MAX_POINTS})")
    out["N"] = N
    return out


class ESC_wave_pc_multires(Dataset):
    """Point sets that hold SEVERAL STFT resolutions at once, framed from the resident waveforms per batch:
    long-window points sharp in frequency and short-window points sharp in time in one (f, t, value) set.
    No reference counterpart (Code/pceval.py:55-105 varies the analysis length one at a time); for a Set
    Transformer it is just a longer set.  One pca_frame_points_multires launch per batch.

    Item idx = set idx of the corpus: clip after clip, L_c // span sets each (``wave_span_offsets``); set s
    of a clip has its anchor at sample s * span.  ``levels`` and the layout of a set: ``multires_layout`` -
    the levels' rows lie back to back in the order given, float32 [N, 3] = (farr_r[f], tarr_r[j], value),
    point ``point_off[r] + j * F_r + f``, with tarr in seconds from the anchor on one clock for all levels;
    ``time_axis=False``: [N, 2] rows (farr_r[f], value), one frame per level.
    ``jitter`` / ``gain_db`` / ``norm`` / ``seed`` as ``ESC_wave_pc``; a batch slot draws one shift, one gain
    and one window INDEX, which every level looks up in its own ``win_lengths``.  Speed change, background
    mix, soft targets, masks and reassignment live in other launches and are not offered here;
    ``PeakPoints`` refuses this dataset (it reads one F x Nt grid).

    ``plain(win_index=0)``: the deterministic view (what the ``Evaluator`` takes); ``with_levels(indices)``:
    a view that keeps only those levels - same span, sets and draws, so a level's rows in the view are its
    rows in the full set.  Views share the resident tensors."""

    batch_seq = None        # augmentations are drawn per call: the Trainer uploads indices per step
    variable_length = False
    soft_targets = False

    def __init__(self, clips, y, fs, levels, span, jitter=0, gain_db=0.0, norm="n_fft", seed=0,
                 device=None, time_axis=True):
        if norm not in ("n_fft", "win"):
            raise ValueError(f"norm is 'n_fft' or 'win', got {norm!r}")
        self.fs, self.span, self.time_axis = fs, int(span), bool(time_axis)
        self.layout = multires_layout(fs, levels, span, self.time_axis)
        self._level_ids = tuple(range(len(self.layout["n_fft"])))       # positions in the resident store
        self.clips, self.clip_labels = list(clips), np.asarray(y).astype(np.int64)
        assert len(self.clips) == len(self.clip_labels) > 0
        self.jitter, self.gain_db = int(jitter), float(gain_db)
        self.norm, self.seed = norm, int(seed)
        self._draw = 0
        self._device = device
        self._store = {}                  # the resident tensors, shared between views
        self.lengths = [int(c.shape[0]) for c in self.clips]
        self._max_len, self._min_len = max(self.lengths), min(self.lengths)
        if self._min_len <= max(self.layout["n_fft"]) // 2:
            raise ValueError(f"multires: the shortest clip ({self._min_len} samples) is no longer than "
                             f"n_fft / 2 of the largest level ({max(self.layout['n_fft']) // 2})")
        self.wave_off = [0] + list(np.cumsum(self.lengths))
        self.set_off = wave_span_offsets(self.lengths, self.span)
        self.labels = np.repeat(self.clip_labels, np.diff(self.set_off))   # label of every set

    def __len__(self):
        return self.set_off[-1]

    @property
    def num_points(self) -> int:
        return self.layout["N"]

    @property
    def stochastic(self) -> bool:
        """True when any augmentation is on: every call must then draw anew, so a caller that captures
        ``batch`` into a hipGraph passes ``draw_dev``."""
        return self.jitter > 0 or self.gain_db > 0.0 or len(self.layout["win_lengths"][0]) > 1

    def plain(self, win_index: int = 0):
        """A view on the same resident waveforms with every augmentation off: deterministic, the anchors
        on the regular grid, every level at its window number ``win_index`` (0: the nominal one)."""
        wins = self.layout["win_lengths"]
        if not 0 <= int(win_index) < len(wins[0]):
            raise ValueError(f"win_index {win_index} outside [0, {len(wins[0])})")
        v = copy.copy(self)
        v.jitter, v.gain_db = 0, 0.0
        v.layout = dict(self.layout, win_lengths=[(w[int(win_index)],) for w in wins])
        v._draw = 0
        return v

    def with_levels(self, indices):
        """A view on the same resident waveforms that keeps only the levels ``indices`` (positions in this
        dataset's levels, in the order given): the same span, sets, labels and draws."""
        indices = [int(k) for k in indices]
        n = len(self._level_ids)
        if not indices or len(set(indices)) != len(indices) or not all(0 <= k < n for k in indices):
            raise ValueError(f"with_levels {indices}: distinct positions in [0, {n})")
        v = copy.copy(self)
        v._level_ids = tuple(self._level_ids[k] for k in indices)
        lay = {k: [val[i] for i in indices] for k, val in self.layout.items() if k != "N"}
        ends = np.cumsum([t * f for t, f in zip(lay["Ntemp"], lay["F"])]).tolist()
        lay["point_off"], lay["N"] = [0] + ends[:-1], ends[-1]
        v.layout = lay
        return v

    def _resident(self):
        """(waves, wave_off, set_off, clip_labels) on the device, uploaded once for all views."""
        if "res" not in self._store:
            dev = _dev(self._device)
            i64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.int64)).to(dev)   # noqa: E731
            waves = torch.cat([torch.as_tensor(c).to(dev, torch.float32).reshape(-1)
                               for c in self.clips])
            self._store["res"] = (waves, i64(self.wave_off), i64(self.set_off), i64(self.clip_labels))
            self._store["axes"], self._store["win"] = {}, {}
        return self._store["res"]

    def _levels_dev(self, dev):
        """The ``pca_hip.FrameLevel`` of every level of this view; axes and window tables are uploaded on
        first use and kept in the shared store (a level's axes do not depend on the view)."""
        f32 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64)).float().to(dev)   # noqa: E731
        lay, out = self.layout, []
        for r, k in enumerate(self._level_ids):
            if k not in self._store["axes"]:
                self._store["axes"][k] = (f32(lay["farr"][r]),
                                          None if lay["tarr"][r] is None else f32(lay["tarr"][r]))
            wkey = (k, lay["win_lengths"][r])
            if wkey not in self._store["win"]:
                self._store["win"][wkey] = torch.tensor(lay["win_lengths"][r], dtype=torch.int32, device=dev)
            f, t = self._store["axes"][k]
            out.append(pca_hip.FrameLevel(lay["n_fft"][r], lay["hop"][r], lay["F"][r], lay["Ntemp"][r], f, t,
                                          self._store["win"][wkey], lay["offset"][r]))
        return out

    def batch(self, idx: torch.Tensor, out=None, labels_out=None, draw_dev=None, want_meta: bool = False):
        """idx int64[B] on the device -> (points [B, num_points, 2 or 3] float32, labels int64[B][, meta
        int32 [B, 8] = (clip, centre sample of level 0's frame 0, level 0's window length, bits of the gain,
        shift, window index, 0, 0)]): one pca_frame_points_multires launch."""
        waves, woff, soff, lab = self._resident()
        self._draw += 1
        return pca_hip.frame_points_multires(
            waves, woff, soff, idx, self._levels_dev(waves.device), self.span, max_len=self._max_len,
            min_len=self._min_len, clip_labels=lab, jitter=self.jitter, gain_db=self.gain_db,
            norm_mode=pca_hip.NORM_WIN if self.norm == "win" else pca_hip.NORM_NFFT, seed=self.seed,
            draw=self._draw, out=out, labels_out=labels_out, draw_dev=draw_dev, want_meta=want_meta)

    def __getitem__(self, idx):
        waves = self._resident()[0]
        pts, lbl = self.batch(torch.tensor([int(idx)], dtype=torch.int64, device=waves.device))
        return pts[0].cpu(), lbl[0].cpu()


class PeakPoints(Dataset):
    """The K strongest spectral peaks of every set of a dense point-set dataset, refined off the grid: a view
    over ``ESC_pc``, ``ESC_pc_temp`` (its variable-length chunks included: their lengths are whole frames),
    ``ESC_wave_pc`` or ``ESC_wave_pc_temp`` with any augmentation but ``mask_mode="drop"``.  No reference
    counterpart: the reference's sets are grid points (all bins, or a subset of them).

    ``batch`` runs the inner dataset's ``batch`` into a dense buffer the view owns (one per batch size, made
    on first use) and ``pca_hip.peak_points`` from there into ``out`` [B, K, din]: two launches.  A set holds
    min(number of peaks, K) rows - at least one: a set without peaks yields its largest point - so the view
    is ``variable_length``: ``batch`` returns (points, labels [, labels2, weight][, sel][, count], lengths)
    and the ``Trainer`` / ``Evaluator`` hand the counts to the step.  K, radius_f, radius_t, rel_floor,
    abs_floor, refine: ``pca_hip.peak_points``."""

    batch_seq = None        # two launches per batch, the second reading the first: indices per step

    def __init__(self, inner, K, radius_f=1, radius_t=0, rel_floor=float("inf"), abs_floor=float("-inf"),
                 refine=True):
        if isinstance(inner, ESC_wave_pc_multires):
            raise ValueError("PeakPoints: a multi-resolution set is several F x Nt grids back to back, and "
                             "peak picking reads its neighbours from one; pick peaks per level "
                             "(ESC_wave_pc / ESC_wave_pc_temp) instead")
        if isinstance(inner, ESC_wave_pc):
            if inner.deltas is not None:
                raise ValueError("PeakPoints: a delta dataset has din > 3 and pca_peak_points takes din 2 or 3; "
                                 "pick peaks on with_deltas(None)")
            self.F, self.Nt, self.din = inner.F, inner._ntemp, 2 if inner.tarr is None else 3
            if inner.variable_length:
                raise ValueError("PeakPoints: mask_mode='drop' removes points from the sets, which breaks "
                                 "the F x Nt grid that peak picking reads its neighbours from; use "
                                 "mask_mode='floor'")
        elif isinstance(inner, ESC_pc_temp) and not isinstance(inner, _TempSS):
            self.F, self.Nt, self.din = int(inner.x.shape[0]), int(inner.x.shape[1]), 3
        elif isinstance(inner, ESC_pc):
            self.F, self.Nt, self.din = int(inner.x.shape[0]), 1, 2
        else:
            raise TypeError(f"PeakPoints needs a dense point-set dataset (ESC_pc, ESC_pc_temp, ESC_wave_pc, "
                            f"ESC_wave_pc_temp), got {type(inner).__name__}")
        self.inner, self.K = inner, int(K)
        if self.F < 3 or not 1 <= self.K <= self.F * self.Nt:
            raise ValueError(f"PeakPoints: F = {self.F} (>= 3), K = {self.K} (1 .. {self.F * self.Nt})")
        pca_hip.ops.peak_spec(radius_f, radius_t, rel_floor, abs_floor, refine)       # ValueError
        self.spec = dict(radius_f=int(radius_f), radius_t=int(radius_t), rel_floor=float(rel_floor),
                         abs_floor=float(abs_floor), refine=bool(refine))
        self._dense = {}                  # B -> (X [B, N, din], lengths int32 [B] or None)

    variable_length = True

    @property
    def num_points(self) -> int:
        return self.K

    @property
    def stochastic(self) -> bool:
        return bool(getattr(self.inner, "stochastic", False))

    @property
    def soft_targets(self) -> bool:
        return bool(getattr(self.inner, "soft_targets", False))

    @property
    def _draw(self):
        """The inner dataset's draw number (the ``Trainer`` checkpoints it and puts it back)."""
        return self.inner._draw

    @_draw.setter
    def _draw(self, value):
        self.inner._draw = value

    @property
    def labels(self):
        return self.inner.labels

    def __len__(self):
        return len(self.inner)

    def _resident(self):
        return self.inner._resident()

    def plain(self, *args, **kw):
        """The view over ``inner.plain()`` (every augmentation off); an inner dataset without one is
        deterministic already and the view itself is returned."""
        if not hasattr(self.inner, "plain"):
            return self
        return PeakPoints(self.inner.plain(*args, **kw), self.K, **self.spec)

    def batch(self, idx: torch.Tensor, out=None, labels_out=None, lengths_out=None, draw_dev=None,
              labels2_out=None, weight_out=None, want_sel: bool = False, want_count: bool = False):
        """idx int64[B] on the device -> (points [B, K, din] float32 - zero rows behind a set's last peak -,
        labels int64[B] [, labels2 int64[B], weight float32[B] with ``soft_targets``][, sel int32 [B, K]]
        [, count int32 [B]], lengths int32 [B])."""
        B = int(idx.numel())
        if B not in self._dense:
            with torch.cuda.device(idx.device):
                self._dense[B] = (
                    torch.empty((B, self.F * self.Nt, self.din), dtype=torch.float32, device=idx.device),
                    torch.zeros(B, dtype=torch.int32, device=idx.device)
                    if getattr(self.inner, "variable_length", False) else None)
        dense, ln = self._dense[B]
        kw = {}
        if ln is not None:
            kw["lengths_out"] = ln
        if isinstance(self.inner, ESC_wave_pc):
            kw["draw_dev"] = draw_dev
            if self.inner.soft_targets:
                kw.update(labels2_out=labels2_out, weight_out=weight_out)
        res = self.inner.batch(idx, out=dense, labels_out=labels_out, **kw)
        soft = tuple(res[2:4]) if self.soft_targets else ()
        peaks = pca_hip.peak_points(dense, self.F, self.Nt, self.K, lengths=ln, out=out,
                                    lengths_out=lengths_out, want_sel=want_sel, want_count=want_count,
                                    **self.spec)
        return (peaks[0], res[1]) + soft + tuple(peaks[2:]) + (peaks[1],)

    def __getitem__(self, idx):
        """The un-padded [lengths, din] rows and the label."""
        dev = self._resident()[0].device
        res = self.batch(torch.tensor([int(idx)], dtype=torch.int64, device=dev))
        return res[0][0, :int(res[-1][0])].cpu(), res[1][0].cpu()


class DeviceBatchLoader:
    """Batches of (points, labels) assembled on the device.

    Replaces ``DataLoader(dataset, batch_size, shuffle=True, num_workers=0)``
    (Code/settransformer.py:71) + ``imgs.to(device)``: the index permutation is drawn on
    the device, rank r of world_size takes indices r::world_size of it
    (DistributedSampler semantics) and each batch is one pack launch.
    """

    def __init__(self, dataset, batch_size: int, shuffle: bool = True, seed: int = 0,
                 rank: int = 0, world_size: int = 1, drop_last: bool = False):
        self.ds, self.bs, self.shuffle = dataset, int(batch_size), shuffle
        self.seed, self.rank, self.world = seed, rank, world_size
        self.drop_last = drop_last
        self.epoch = 0

    def set_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def _indices(self) -> torch.Tensor:
        dev = self.ds._resident()[0].device
        n = len(self.ds)
        if self.shuffle:
            g = torch.Generator(device="cpu").manual_seed(self.seed + self.epoch)
            perm = torch.randperm(n, generator=g).to(dev)
        else:
            perm = torch.arange(n, device=dev)
        per = n // self.world                      # equal share per rank (tail dropped)
        return perm[self.rank:per * self.world:self.world].contiguous()

    def __len__(self) -> int:
        per = len(self.ds) // self.world
        return per // self.bs if self.drop_last else -(-per // self.bs)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        idx = self._indices()
        n = idx.numel()
        stop = (n // self.bs) * self.bs if self.drop_last else n
        for s in range(0, stop, self.bs):
            yield self.ds.batch(idx[s:s + self.bs])
