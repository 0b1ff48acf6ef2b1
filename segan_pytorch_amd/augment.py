"""On-the-fly additive noise at a target SNR on the MI355X: the reference's
`Additive` (segan/utils.py:43-297) with the level measurement (ITU-T P.56 method B) and the mix as
HIP kernels (`ops.asl_p56`, `ops.additive_mix`), batched.  And on-the-fly reverberation (section
14): `Reverb` convolves each row with a room impulse response of an `RIRBank`
(`ops.reverb_rows`)."""
import glob
import os

import numpy as np
import torch

from . import ops


class NoiseBank(object):
    """Noise recordings concatenated into one flat fp32 array with per-file offsets; the device
    copy is made on first use.  `NoiseBank(list_of_arrays)` takes float arrays as they are and
    int16 arrays as int16 / 32768; `NoiseBank.from_dir(dir)` reads every *.wav of a directory
    (16-bit PCM -> int16 / 32768, which is what the reference's `librosa.load(sr=None)` yields;
    multi-channel files are averaged as librosa does).  The rate in the headers is ignored unless
    `from_dir(dir, target_rate=16000)` is given: files of another rate are then converted to it on
    the GPU first (`resample.resample_many`: int16 -> int16, channels averaged before)."""

    def __init__(self, arrays, files=None):
        arrays = [self._as_float(a) for a in arrays]
        if len(arrays) == 0:
            raise ValueError('[!] No noises found in {}'.format(files if files is not None else arrays))
        self.files = list(files) if files is not None else ['noise{}'.format(i)
                                                            for i in range(len(arrays))]
        self.lengths = np.array([len(a) for a in arrays], dtype=np.int64)
        if (self.lengths == 0).any():
            raise ValueError('NoiseBank: empty noise array')
        self.offsets = np.concatenate(([0], np.cumsum(self.lengths))).astype(np.int64)
        self.host = np.concatenate(arrays)
        self._dev = {}

    @staticmethod
    def _as_float(a):
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        if a.dtype == np.int16:
            a = a.astype(np.float32) / np.float32(32768)
        elif not np.issubdtype(a.dtype, np.floating):
            raise TypeError('NoiseBank: noises must be float or int16 arrays, got {}'.format(a.dtype))
        if a.ndim == 2:      # [samples, channels] as scipy reads it
            a = a.mean(axis=1)
        return np.ascontiguousarray(a.reshape(-1), dtype=np.float32)

    @classmethod
    def from_dir(cls, noises_dir, target_rate=None, resample_zeros=ops.RESAMPLE_ZEROS,
                 resample_beta=ops.RESAMPLE_BETA):
        from scipy.io import wavfile
        names = sorted(glob.glob(os.path.join(noises_dir, '*.wav')))
        if len(names) == 0:
            raise ValueError('[!] No noises found in {}'.format(noises_dir))
        read = [wavfile.read(n) for n in names]
        wavs = [w for _, w in read]
        if target_rate is not None:
            from .resample import resample_many
            wavs, _ = resample_many(wavs, [r for r, _ in read], target_rate, resample_zeros,
                                    resample_beta)
        return cls(wavs, files=names)

    def __len__(self):
        return len(self.lengths)

    def data(self, device):
        """The flat bank on `device` (a HIP device; uploaded once per device)."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('NoiseBank: segan_pytorch_amd runs only on an MI355X (HIP) device; '
                               'there is no CPU path')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.host).to(device)
        return self._dev[device]

    def draw(self, rng, sig_lengths, snr_levels, noise_ids=None, snrs=None, starts=None):
        """Per row, from the numpy Generator `rng`: a noise file (uniform), an SNR level (uniform
        over `snr_levels`) and a start uniform over the file's valid starts 1 .. len(file) -
        len(signal) — a segment never straddles two files.  The rows' files are drawn first, then
        their levels, then their starts (three vectorised draws); values passed in are kept and
        not drawn.  Returns (noise_ids, snrs, starts) as numpy arrays, starts relative to the
        file.  A noise no longer than the signal raises the reference's ValueError."""
        sig_lengths = np.asarray(sig_lengths, dtype=np.int64).reshape(-1)
        rows = len(sig_lengths)
        if starts is not None and noise_ids is None:
            raise ValueError('Additive: starts are offsets into a noise file; pass noise_ids too')
        if noise_ids is None:
            ids = rng.integers(len(self), size=rows)
        else:
            ids = np.asarray(noise_ids, dtype=np.int64).reshape(-1)
            if len(ids) != rows or (ids < 0).any() or (ids >= len(self)).any():
                raise ValueError('Additive: {} noise ids in 0 .. {} expected, got {}'.format(
                    rows, len(self) - 1, ids.tolist()))
        if snrs is None:
            sn = np.asarray(snr_levels, dtype=np.float64)[rng.integers(len(snr_levels), size=rows)]
        else:
            sn = np.asarray(snrs, dtype=np.float64).reshape(-1)
            if len(sn) != rows:
                raise ValueError('Additive: {} snrs expected, got {}'.format(rows, len(sn)))
        limit = self.lengths[ids] - sig_lengths      # the last valid start
        if (limit < 1).any():
            r = int(np.nonzero(limit < 1)[0][0])
            raise ValueError('Noise length has to be greater than speech length! (noise {}: {}, '
                             'speech: {})'.format(self.files[ids[r]], self.lengths[ids[r]],
                                                  sig_lengths[r]))
        if starts is None:
            st = rng.integers(1, limit + 1)
        else:
            st = np.asarray(starts, dtype=np.int64).reshape(-1)
            if len(st) != rows or (st < 1).any() or (st > limit).any():
                r = 0 if len(st) != rows else int(np.nonzero((st < 1) | (st > limit))[0][0])
                raise ValueError('Additive: start {} outside 1 .. {} of noise {}'.format(
                    st[r] if len(st) == rows else st.tolist(), limit[r], self.files[ids[r]]))
        return ids.astype(np.int64), sn, st.astype(np.int64)


class Additive(object):
    """The reference's `Additive(noises_dir, snr_levels, do_IRS)` on the GPU.  `noises`: a
    directory of wavs, a list of arrays or a `NoiseBank`.  `__call__(wav)` mixes one waveform like
    the reference and returns a CPU FloatTensor; `mix(clean[B, T])` mixes a batch on the device.

    Per waveform: Px = the P.56 active-level mean square of the clean signal, Pn = the mean square
    of the drawn noise segment, sf = sqrt(Px / Pn / 10^(snr/10)), noisy = clean + sf * segment,
    then the reference's anti-clipping divisions (by 1.1, 1.2, ... while max >= 1 or min < -1).

    Draws come from a numpy Generator owned by the object (`seed`), not from numpy's global
    state.  Departures from the reference, all on inputs where the reference fails:
      * its start draw `round((limit - 1) * rand + 1)` can select the start one past the last
        valid one and then fails on the short slice; here the start is uniform over the valid
        starts 1 .. len(noise) - len(signal);
      * Px == 0 (silence, or a level below the P.56 margin) gives sf = 0 and noisy == clean, as
        the reference's arithmetic does;
      * Pn == 0 (a segment of digital silence; inf / NaN in the reference) gives noisy == clean,
        flagged in info['status'] (ops.ADDITIVE_PN0).
    `do_IRS=True` raises NotImplementedError, as the reference's `apply_IRS` does.  `target_rate`
    (with a directory): noise files of another rate are converted to it on the GPU when they are
    read (`NoiseBank.from_dir`); without it their rate is ignored."""

    def __init__(self, noises, snr_levels=[0, 5, 10], do_IRS=False, seed=None, target_rate=None):
        if do_IRS:
            raise NotImplementedError('Under construction!')
        if isinstance(noises, NoiseBank):
            self.bank = noises
        elif isinstance(noises, (str, os.PathLike)):
            self.noises_dir = noises
            self.bank = NoiseBank.from_dir(noises, target_rate=target_rate)
        else:
            self.bank = NoiseBank(noises)
        if len(snr_levels) == 0:
            raise ValueError('Additive: snr_levels is empty')
        self.snr_levels = list(snr_levels)
        self.do_IRS = do_IRS
        self.rng = np.random.default_rng(seed)

    def mix(self, clean, generator=None, starts=None, snrs=None, noise_ids=None, srate=16000,
            lengths=None, prev=None):
        """clean [B, T] (fp32 CUDA) -> (noisy [B, T], info).  `generator`: a numpy Generator used
        instead of the object's; `noise_ids`, `snrs`, `starts` (per row; starts are offsets into
        the row's noise file and need noise_ids) replace the corresponding draws.  info: the
        dict of `ops.additive_mix` plus asl_ms, asl, c0 (device) and noise_ids, snrs, starts,
        abs_starts (numpy, host)."""
        ops._chk(clean, 'clean', 2)
        rows, T = clean.shape
        rng = self.rng if generator is None else generator
        sig = np.full(rows, T, dtype=np.int64) if lengths is None else np.asarray(
            torch.as_tensor(lengths).cpu(), dtype=np.int64)
        ids, sn, st = self.bank.draw(rng, sig, self.snr_levels, noise_ids, snrs, starts)
        level = ops.asl_p56(clean, srate, 16, lengths)
        ab = self.bank.offsets[ids] + st
        noisy, info = ops.additive_mix(clean, self.bank.data(clean.device), ab, sn, level['asl_ms'],
                                       lengths, prev)
        info.update(asl_ms=level['asl_ms'], asl=level['asl'], c0=level['c0'], noise_ids=ids, snrs=sn,
                    starts=st, abs_starts=ab)
        return noisy, info

    def __call__(self, wav, srate=16000, nbits=16):
        """Add noise to one clean waveform (numpy array or tensor, any shape: flattened)."""
        if nbits != 16:
            raise NotImplementedError('Additive: nbits={} is not supported (16 only)'.format(nbits))
        if not torch.cuda.is_available():
            raise RuntimeError('segan_pytorch_amd runs only on an MI355X (HIP) device; there is no '
                               'CPU path')
        if isinstance(wav, torch.Tensor):
            wav = wav.detach().cpu().numpy()
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(wav, dtype=np.float32).reshape(1, -1)))
        noisy, _ = self.mix(x.cuda(), srate=srate)
        return noisy[0].cpu().type(torch.FloatTensor)


class RIRBank(object):
    """Room impulse responses, normalised once on the host in float64: each is cut to `max_taps`,
    d = argmax |h| (first occurrence) is its direct path, h / h[d] is rounded to fp32 once — the
    direct path stays time-aligned with the dry signal and has gain exactly 1 (a negative peak
    divides through).  An RIR without a non-zero tap is refused.  `RIRBank(list_of_arrays)` takes
    arrays as `NoiseBank` does; `RIRBank.from_dir(dir)` reads every *.wav of a directory with the
    same reader and the same optional GPU rate conversion (`target_rate`).

    `taps`, `delays`: int64 arrays, per RIR.  `data(device)`: the bank on a HIP device, built on
    first use — the spectra of the RIRs' partitions (`ops.reverb_bank`: P = ops.REVERB_P taps each,
    8 bytes per tap of the RIR padded to a multiple of P, 128 KiB for 16384 taps) and the
    per-RIR table (first partition, partitions, taps, d)."""

    def __init__(self, arrays, files=None, max_taps=16384):
        max_taps = int(max_taps)
        if max_taps < 1:
            raise ValueError('RIRBank: max_taps must be positive, got {}'.format(max_taps))
        arrays = list(arrays)
        if len(arrays) == 0:
            raise ValueError('[!] No impulse responses found in {}'.format(
                files if files is not None else arrays))
        self.files = list(files) if files is not None else ['rir{}'.format(i)
                                                            for i in range(len(arrays))]
        self.max_taps = max_taps
        self.rirs, delays = [], []
        for name, a in zip(self.files, arrays):
            h, d = self._normalise(self._as_float64(a), max_taps, name)
            self.rirs.append(h)
            delays.append(d)
        self.taps = np.array([len(h) for h in self.rirs], dtype=np.int64)
        self.delays = np.array(delays, dtype=np.int64)
        P = ops.REVERB_P
        self.partitions = (self.taps + P - 1) // P
        self.offsets = np.concatenate(([0], np.cumsum(self.partitions))).astype(np.int64)
        if int(self.offsets[-1]) >= 1 << 31:
            raise ValueError('RIRBank: {} partitions do not fit the table'.format(self.offsets[-1]))
        self._dev = {}

    @staticmethod
    def _as_float64(a):
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        if a.dtype == np.int16:
            a = a.astype(np.float64) / 32768.0
        elif not np.issubdtype(a.dtype, np.floating):
            raise TypeError('RIRBank: impulse responses must be float or int16 arrays, got {}'.format(
                a.dtype))
        if a.ndim == 2:      # [samples, channels] as scipy reads it
            a = a.astype(np.float64).mean(axis=1)
        return np.ascontiguousarray(a.reshape(-1), dtype=np.float64)

    @staticmethod
    def _normalise(h, max_taps, name):
        # restated by scripts/reverb_oracle.py:normalise (the oracle's copy): keep the two alike
        h = h[:max_taps]
        if h.size == 0 or not np.any(h != 0):
            raise ValueError('RIRBank: {} has no non-zero tap within max_taps={}'.format(
                name, max_taps))
        if not np.all(np.isfinite(h)):
            raise ValueError('RIRBank: {} has a non-finite tap'.format(name))
        d = int(np.argmax(np.abs(h)))
        return (h / h[d]).astype(np.float32), d

    @classmethod
    def from_dir(cls, rirs_dir, target_rate=None, max_taps=16384, resample_zeros=ops.RESAMPLE_ZEROS,
                 resample_beta=ops.RESAMPLE_BETA):
        from scipy.io import wavfile
        names = sorted(glob.glob(os.path.join(rirs_dir, '*.wav')))
        if len(names) == 0:
            raise ValueError('[!] No impulse responses found in {}'.format(rirs_dir))
        read = [wavfile.read(n) for n in names]
        wavs = [w for _, w in read]
        if target_rate is not None:
            from .resample import resample_many
            wavs, _ = resample_many(wavs, [r for r, _ in read], target_rate, resample_zeros,
                                    resample_beta)
        return cls(wavs, files=names, max_taps=max_taps)

    def __len__(self):
        return len(self.rirs)

    def padded(self):
        """The RIRs zero-padded to whole partitions and concatenated: fp32 [partitions, P]."""
        P = ops.REVERB_P
        out = np.zeros((int(self.offsets[-1]), P), dtype=np.float32)
        flat = out.reshape(-1)
        for h, o in zip(self.rirs, self.offsets[:-1]):
            flat[o * P:o * P + len(h)] = h
        return out

    def data(self, device):
        """`ops.ReverbBankData` of the bank on `device` (a HIP device; built once per device)."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('RIRBank: segan_pytorch_amd runs only on an MI355X (HIP) device; '
                               'there is no CPU path')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device not in self._dev:
            with torch.cuda.device(device):
                H = ops.reverb_bank(torch.from_numpy(self.padded()).to(device))
                table = np.stack([self.offsets[:-1], self.partitions, self.taps, self.delays], axis=1)
                table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(device)
                torch.cuda.current_stream(device).synchronize()      # other streams use it next
            self._dev[device] = ops.ReverbBankData(H, table, int(self.delays.max()))
        return self._dev[device]


class Reverb(object):
    """On-the-fly reverberation.  `rirs`: a directory of wavs, a list of
    arrays or an `RIRBank`.  `apply(clean[B, T])` convolves each row with an RIR drawn uniformly
    from the bank, on the device; `__call__(wav)` does one waveform and returns a CPU FloatTensor,
    like `Additive.__call__`.  The direct path of every RIR has gain 1 and stays aligned with the
    dry signal, which remains the regression target.  Every slice is reverberated as if silence
    preceded it: no tail is carried over from earlier slices of the utterance.  Draws come from a
    numpy Generator owned by the object (`seed`)."""

    def __init__(self, rirs, seed=None, max_taps=16384, target_rate=None):
        if isinstance(rirs, RIRBank):
            self.bank = rirs
        elif isinstance(rirs, (str, os.PathLike)):
            self.rirs_dir = rirs
            self.bank = RIRBank.from_dir(rirs, target_rate=target_rate, max_taps=max_taps)
        else:
            self.bank = RIRBank(rirs, max_taps=max_taps)
        self.rng = np.random.default_rng(seed)

    def draw(self, rng, rows, rir_ids=None):
        if rir_ids is None:
            return rng.integers(len(self.bank), size=rows).astype(np.int64)
        ids = np.asarray(rir_ids, dtype=np.int64).reshape(-1)
        if len(ids) != rows or (ids < 0).any() or (ids >= len(self.bank)).any():
            raise ValueError('Reverb: {} rir ids in 0 .. {} expected, got {}'.format(
                rows, len(self.bank) - 1, ids.tolist()))
        return ids

    def apply(self, clean, generator=None, rir_ids=None, lengths=None, prev=None):
        """clean [B, T] (fp32 CUDA) -> (wet [B, T], info).  `generator`: a numpy Generator used
        instead of the object's; `rir_ids` (per row) replaces the draw.  info: rir_ids, taps,
        delays (numpy, host), prev (device: the reverberant sample preceding each row) and status
        (device int32, `ops.reverb_rows`)."""
        ops._chk(clean, 'clean', 2)
        ids = self.draw(self.rng if generator is None else generator, clean.shape[0], rir_ids)
        wet, info = ops.reverb_rows(clean, self.bank, ids, lengths, prev)
        info.update(rir_ids=ids, taps=self.bank.taps[ids], delays=self.bank.delays[ids])
        return wet, info

    def __call__(self, wav):
        """Reverberate one waveform (numpy array or tensor, any shape: flattened)."""
        if not torch.cuda.is_available():
            raise RuntimeError('segan_pytorch_amd runs only on an MI355X (HIP) device; there is no '
                               'CPU path')
        if isinstance(wav, torch.Tensor):
            wav = wav.detach().cpu().numpy()
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(wav, dtype=np.float32).reshape(1, -1)))
        wet, _ = self.apply(x.cuda())
        return wet[0].cpu().type(torch.FloatTensor)


class ComposeAdditive(object):
    """utils.py:43-49: x -> (x, additive(x))."""

    def __init__(self, additive):
        self.additive = additive

    def __call__(self, x):
        return x, self.additive(x)
