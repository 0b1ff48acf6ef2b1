"""On-the-fly additive noise at a target SNR on the MI355X: the reference's
`Additive` (segan/utils.py:43-297) with the level measurement (ITU-T P.56 method B) and the mix as
HIP kernels (`ops.asl_p56`, `ops.additive_mix`), batched.  And on-the-fly reverberation (section
14): `Reverb` convolves each row with a room impulse response of an `RIRBank`
(`ops.reverb_rows`).  And three signal-level distortions (section 17): `Clip` (amplitude clipping,
`ops.clip_rows`), `Chop` (chunks of speech removed, `ops.chop_rows`), `BandLimit` (a zero-phase
low-pass, `ops.fir_rows`), and `Distort`, which applies one of them per row.  And whispered speech
(section 18): `Whisper` replaces the voiced excitation by noise under the same spectral envelope
(`ops.whisper_rows`).  And synthetic rooms (section 24): `draw_rooms` and `RIRBank.synthetic` make a
bank of shoebox-room responses by the image-source method (`ops.rir_shoebox`), so that `Reverb`
needs no measured responses."""
import glob
import os

import numpy as np
import torch

from . import ops


def _one_wave(run, wav, **kw):
    """What every `__call__(wav)` here does: one waveform (numpy array or tensor, any shape:
    flattened) goes through the batched `run` (an `apply` or `mix`) as a batch of one row on the
    device, and that row comes back as a CPU FloatTensor."""
    if not torch.cuda.is_available():
        raise RuntimeError('segan_pytorch_amd runs only on an MI355X (HIP) device; there is no '
                           'CPU path')
    if isinstance(wav, torch.Tensor):
        wav = wav.detach().cpu().numpy()
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(wav, dtype=np.float32).reshape(1, -1)))
    out, _ = run(x.cuda(), **kw)
    return out[0].cpu().type(torch.FloatTensor)


def _on_device(owner, device, build):
    """owner._dev[device]: what `build(device)` returns, built once per device with that device
    current.  `device` must be a HIP device; 'cuda' alone is the current one."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('{}: segan_pytorch_amd runs only on an MI355X (HIP) device; there is no '
                           'CPU path'.format(type(owner).__name__))
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    if device not in owner._dev:
        with torch.cuda.device(device):
            owner._dev[device] = build(device)
    return owner._dev[device]


def _draw_ids(rng, n, rows, ids, who, noun):
    """One id in 0 .. n - 1 per row, uniform (one vectorised draw from `rng`); `ids` given are
    checked, kept and not drawn.  `who` and `noun` name them in the message."""
    if ids is None:
        return rng.integers(n, size=rows).astype(np.int64)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if len(ids) != rows or (ids < 0).any() or (ids >= n).any():
        raise ValueError('{}: {} {} in 0 .. {} expected, got {}'.format(who, rows, noun, n - 1,
                                                                         ids.tolist()))
    return ids


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
        return _on_device(self, device, lambda dev: torch.from_numpy(self.host).to(dev))

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
        ids = _draw_ids(rng, len(self), rows, noise_ids, 'Additive', 'noise ids')
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
        return ids, sn, st.astype(np.int64)


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
        return _one_wave(self.mix, wav, srate=srate)


def beta_from_rt60(room, rt60):
    """One reflection coefficient for all six walls of a shoebox `room` ([.., 3] metres) from a
    nominal reverberation time `rt60` (seconds) by Sabine's formula: the mean absorption is
    (24 ln 10 / c) V / (S rt60) with c = 343 m/s, and beta = sqrt(max(1 - absorption, 0)).  Nominal:
    the image-source response of such a room decays more slowly than diffuse-field theory says, its
    Schroeder T30 was 1.2 to 1.4 times `rt60` where measured."""
    room = np.asarray(room, np.float64)
    rt60 = np.asarray(rt60, np.float64)
    if room.shape[-1:] != (3,) or np.any(room <= 0) or np.any(rt60 <= 0):
        raise ValueError('beta_from_rt60: positive sides [.., 3] and a positive rt60 expected')
    lx, ly, lz = room[..., 0], room[..., 1], room[..., 2]
    volume = lx * ly * lz
    surface = 2.0 * (lx * ly + ly * lz + lx * lz)
    absorption = (24.0 * np.log(10.0) / ops.RIR_C) * volume / (surface * rt60)
    return np.sqrt(np.maximum(1.0 - absorption, 0.0))


def draw_rooms(rng, count, rt60=(0.2, 0.8), room_min=(3, 3, 2.5), room_max=(10, 8, 4),
               wall_margin=0.5, min_dist=0.5):
    """`count` shoebox rooms from the numpy Generator `rng`, host only.  Room after room, every
    draw uniform and in this order: the nominal rt60 in [rt60[0], rt60[1]]; the three sides in
    [room_min, room_max]; then the three coordinates of the source and the three of the receiver,
    each in [wall_margin, side - wall_margin], the six drawn again until the two are at least
    `min_dist` metres apart.  Returns a dict of fp64 arrays: 'room', 'src', 'mic' [count, 3],
    'rt60' [count] and 'beta' [count, 6] (`beta_from_rt60`, the same on the six walls)."""
    count = int(count)
    lo, hi = float(rt60[0]), float(rt60[1])
    rmin, rmax = np.asarray(room_min, np.float64), np.asarray(room_max, np.float64)
    margin, min_dist = float(wall_margin), float(min_dist)
    if count < 1 or not 0 < lo <= hi:
        raise ValueError('draw_rooms: count >= 1 and 0 < rt60[0] <= rt60[1] expected')
    if rmin.shape != (3,) or rmax.shape != (3,) or np.any(rmin > rmax) or margin <= 0:
        raise ValueError('draw_rooms: room_min <= room_max (three sides each) and a positive '
                         'wall_margin expected')
    inner = rmin - 2.0 * margin
    if np.any(inner <= 0) or min_dist <= 0 or np.sqrt(np.sum(inner ** 2)) < 2.0 * min_dist:
        raise ValueError('draw_rooms: the smallest room leaves no space for a source and a '
                         'receiver {} m apart, {} m from the walls'.format(min_dist, margin))
    out = dict(room=np.zeros((count, 3)), src=np.zeros((count, 3)), mic=np.zeros((count, 3)),
               rt60=np.zeros(count))
    for i in range(count):
        out['rt60'][i] = rng.uniform(lo, hi)
        room = rng.uniform(rmin, rmax)
        while True:
            src = rng.uniform(margin, room - margin)
            mic = rng.uniform(margin, room - margin)
            if np.sqrt(np.sum((src - mic) ** 2)) >= min_dist:
                break
        out['room'][i], out['src'][i], out['mic'][i] = room, src, mic
    out['beta'] = np.repeat(beta_from_rt60(out['room'], out['rt60'])[:, None], 6, axis=1)
    return out


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

    @classmethod
    def synthetic(cls, count, seed, device, max_taps=16384, srate=16000, **draw):
        """A bank of `count` image-source responses of rooms drawn by `draw_rooms` (its keyword
        arguments in `draw`) from numpy.random.default_rng(seed), synthesised on `device` (a HIP
        device) at `srate`: row i is ceil(1.5 rt60_i srate) taps long, `max_taps` at the most.  The
        rows go through the constructor like any others; `rooms` keeps what `draw_rooms` gave."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('RIRBank: segan_pytorch_amd runs only on an MI355X (HIP) device; '
                               'there is no CPU path')
        max_taps = int(max_taps)
        if max_taps < 1:
            raise ValueError('RIRBank: max_taps must be positive, got {}'.format(max_taps))
        rooms = draw_rooms(np.random.default_rng(seed), count, **draw)
        lengths = np.minimum(max_taps, np.ceil(1.5 * rooms['rt60'] * srate)).astype(np.int64)
        with torch.cuda.device(device):
            h = ops.rir_shoebox(rooms['room'], rooms['src'], rooms['mic'], rooms['beta'],
                                int(lengths.max()), srate=srate, lengths=lengths).cpu().numpy()
        bank = cls([h[i, :n] for i, n in enumerate(lengths)],
                   files=['synthetic{}'.format(i) for i in range(len(lengths))], max_taps=max_taps)
        bank.rooms = rooms
        return bank

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
        def build(dev):
            H = ops.reverb_bank(torch.from_numpy(self.padded()).to(dev))
            table = np.stack([self.offsets[:-1], self.partitions, self.taps, self.delays], axis=1)
            table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(dev)
            torch.cuda.current_stream(dev).synchronize()      # other streams use it next
            return ops.ReverbBankData(H, table, int(self.delays.max()))

        return _on_device(self, device, build)


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
        return _draw_ids(rng, len(self.bank), rows, rir_ids, 'Reverb', 'rir ids')

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
        return _one_wave(self.apply, wav)


# ---------------------------------------------------------------------------------
# clipping, chunk removal and band limiting.  Every default below is this
# project's own choice, not taken from a paper.
# ---------------------------------------------------------------------------------
DISTORT_KINDS = ('clip', 'chop', 'bandlimit')


class _RowDistortion(object):
    """What Clip, Chop and BandLimit share: draws from a numpy Generator owned by the object
    (`seed`), and `__call__(wav)` on one waveform (numpy array or tensor, any shape: flattened),
    which returns a CPU FloatTensor like `Reverb.__call__`."""

    def __call__(self, wav):
        return _one_wave(self.apply, wav)


class Clip(_RowDistortion):
    """Amplitude clipping at `factor` times the row's own peak, one factor per row drawn uniformly
    from `factors` (each in (0, 1]; 1.0 changes nothing)."""
    kind = 'clip'

    def __init__(self, factors=(0.1, 0.2, 0.3, 0.4, 0.5), seed=None):
        self.factors = np.asarray(list(factors), dtype=np.float64).reshape(-1)
        if len(self.factors) == 0 or not ((self.factors > 0) & (self.factors <= 1)).all():
            raise ValueError('Clip: factors must be non-empty and lie in (0, 1], got {}'.format(
                list(factors)))
        self.rng = np.random.default_rng(seed)

    def draw(self, rng, rows, factors=None):
        """One factor per row (one vectorised draw); `factors` given are kept and not drawn."""
        if factors is None:
            return self.factors[rng.integers(len(self.factors), size=rows)]
        f = np.asarray(factors, dtype=np.float64).reshape(-1)
        if len(f) != rows or not ((f > 0) & (f <= 1)).all():
            raise ValueError('Clip: {} factors in (0, 1] expected, got {}'.format(rows, f.tolist()))
        return f

    def apply(self, wave, generator=None, factors=None, lengths=None, prev=None):
        """wave [B, T] (fp32 CUDA) -> (clipped [B, T], info).  info: the dict of `ops.clip_rows`
        (m, thr, nclipped, status, and prev — the clamped sample preceding each row — when `prev`
        is given) plus factors (numpy, host)."""
        ops._chk(wave, 'wave', 2)
        f = self.draw(self.rng if generator is None else generator, wave.shape[0], factors)
        out, info = ops.clip_rows(wave, f, lengths, prev)
        info.update(factors=f)
        return out, info


class Chop(_RowDistortion):
    """Chunks of speech removed (dropouts): per row 1 .. `max_chops` chunks, each `durs[0]` ..
    `durs[1]` seconds long, start where the P.56 envelope of the row is above its activity
    threshold (`ops.asl_p56_stages`: q >= c0), so that speech and not a pause is hit.  A row
    without a P.56 level (silence, or a level below the margin) is left unchanged
    (ops.CHOP_NOLEVEL)."""
    kind = 'chop'

    def __init__(self, max_chops=3, durs=(0.05, 0.3), srate=16000, seed=None):
        self.max_chops = ops._int_arg(max_chops, 'Chop: max_chops', 1, ops.CHOP_MAX)
        self.srate = ops._int_arg(srate, 'Chop: srate', 1, 768000)
        lo, hi = (float(d) for d in durs)
        if not (0.0 < lo <= hi) or hi * self.srate >= 2 ** 31 or np.rint(lo * self.srate) < 1:
            raise ValueError('Chop: durs must be 0 < lo <= hi seconds and at least a sample, got '
                             '{}'.format(list(durs)))
        self.durs = (lo, hi)
        self.rng = np.random.default_rng(seed)

    def draw(self, rng, rows):
        """(u float64 [rows, max_chops], dur int32 [rows, max_chops]) from three vectorised draws
        in this order: the rows' chunk counts (uniform over 1 .. max_chops), max_chops durations per
        row (uniform over `durs`, rounded to samples) and max_chops positions u per row (uniform
        over [0, 1)).  The slots from a row's count on are unused (dur = 0): every row consumes
        the same number of draws whatever its count."""
        C = self.max_chops
        count = rng.integers(1, C + 1, size=rows)
        dur = np.rint(rng.uniform(self.durs[0], self.durs[1], size=(rows, C)) * self.srate)
        u = rng.random((rows, C))
        dur = np.where(np.arange(C)[None, :] < count[:, None], dur, 0).astype(np.int32)
        return u, dur

    def apply(self, wave, generator=None, u=None, dur=None, lengths=None, prev=None):
        """wave [B, T] (fp32 CUDA) -> (chopped [B, T], info).  `u`, `dur` ([B, C], both or
        neither) replace the draws.  info: the dict of `ops.chop_rows` (starts, nactive, nzeroed,
        status) plus c0 (device), u, dur (numpy, host) and prev: the incoming `prev`, untouched
        (when given)."""
        ops._chk(wave, 'wave', 2)
        if (u is None) != (dur is None):
            raise ValueError('Chop: u and dur go together')
        if u is None:
            u, dur = self.draw(self.rng if generator is None else generator, wave.shape[0])
        level = ops.asl_p56_stages(wave, self.srate, 16, lengths)
        out, info = ops.chop_rows(wave, level['q'], level['c0'], u, dur, lengths)
        info.update(c0=level['c0'], u=u, dur=dur)
        if prev is not None:
            info['prev'] = prev
        return out, info


def lowpass_bank(cutoffs, srate=16000, zeros=32, beta=8.6):
    """(bank float64 [nf, Kmax + 1], K int32 [nf]): per cutoff fc (Hz) the one-sided taps of a
    zero-phase Kaiser-windowed sinc low-pass, built on the host in float64: K = ceil(zeros srate /
    (2 fc)), h[k] = sinc(2 fc k / srate) w(k) with w the Kaiser window of half-length K and
    parameter beta, scaled so that h[0] + 2 sum_{k>=1} h[k] = 1 (unit gain at DC; -6 dB at fc).
    Rows are zero after their own K.  K > ops.FIR_MAX_K (a cutoff too low for `zeros`) raises
    ValueError.  Restated by scripts/distort_oracle.py:lowpass: keep the two alike."""
    fcs = np.asarray(list(cutoffs), dtype=np.float64).reshape(-1)
    if len(fcs) == 0 or not ((fcs > 0) & (fcs < srate / 2.0)).all():
        raise ValueError('lowpass_bank: cutoffs must be non-empty and lie in (0, {}) Hz, got '
                         '{}'.format(srate / 2.0, fcs.tolist()))
    if not (zeros >= 1 and 0.0 <= beta <= ops.RESAMPLE_BETA_MAX):
        raise ValueError('lowpass_bank: zeros >= 1 and beta in 0 .. {} expected, got {}, {}'.format(
            ops.RESAMPLE_BETA_MAX, zeros, beta))
    Ks = [int(np.ceil(zeros * srate / (2.0 * fc))) for fc in fcs]
    if max(Ks) > ops.FIR_MAX_K:
        raise ValueError('lowpass_bank: cutoff {} Hz needs K = {} > {} taps a side'.format(
            fcs[int(np.argmax(Ks))], max(Ks), ops.FIR_MAX_K))
    bank = np.zeros((len(fcs), max(Ks) + 1), dtype=np.float64)
    for f, (fc, K) in enumerate(zip(fcs, Ks)):
        k = np.arange(K + 1, dtype=np.float64)
        w = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (k / K) ** 2))) / np.i0(beta)
        h = np.sinc(2.0 * fc * k / srate) * w
        bank[f, :K + 1] = h / (h[0] + 2.0 * h[1:].sum())
    return bank, np.asarray(Ks, dtype=np.int32)


class BandLimit(_RowDistortion):
    """Bandwidth reduction: each row is low-pass filtered at a cutoff drawn uniformly from
    `cutoffs` (Hz) with a zero-phase FIR of `lowpass_bank`; the sample rate stays what it is."""
    kind = 'bandlimit'

    def __init__(self, cutoffs=(1000, 2000, 4000), srate=16000, zeros=32, beta=8.6, seed=None):
        self.cutoffs = np.asarray(list(cutoffs), dtype=np.float64).reshape(-1)
        self.bank, self.K = lowpass_bank(self.cutoffs, srate, zeros, beta)
        self.srate = srate
        self.rng = np.random.default_rng(seed)
        self._dev = {}

    def data(self, device):
        """(bank, K) on `device` (a HIP device; uploaded once per device)."""
        def build(dev):
            pair = (torch.from_numpy(self.bank).to(dev), torch.from_numpy(self.K).to(dev))
            torch.cuda.current_stream(dev).synchronize()      # other streams use it next
            return pair

        return _on_device(self, device, build)

    def draw(self, rng, rows, ids=None):
        return _draw_ids(rng, len(self.cutoffs), rows, ids, 'BandLimit', 'filter ids')

    def apply(self, wave, generator=None, ids=None, lengths=None, prev=None, out_dtype=None):
        """wave [B, T] (fp32 CUDA) -> (filtered [B, T], info).  `ids` (per row) replaces the draw.
        info: the dict of `ops.fir_rows` (prev = the filtered sample preceding each row, status)
        plus ids, cutoffs (numpy, host)."""
        ops._chk(wave, 'wave', 2)
        ids = self.draw(self.rng if generator is None else generator, wave.shape[0], ids)
        bank, K = self.data(wave.device)
        out, info = ops.fir_rows(wave, bank, K, ids, lengths, prev, out_dtype)
        info.update(ids=ids, cutoffs=self.cutoffs[ids])
        return out, info


class Distort(object):
    """One of several distortions per row.  `kinds`: a list of `Clip` / `Chop` / `BandLimit`
    objects, or a dict {'clip': ..., 'chop': ..., 'bandlimit': ...}; at most one of each.  `apply`
    draws, from ONE generator and in this fixed order:
      1. the kind of every row, uniform among the enabled kinds (one vectorised draw; the enabled
         kinds are numbered in the order clip, chop, bandlimit);
      2. clip's draws for its rows, in ascending row order (`Clip.draw`);
      3. chop's draws for its rows likewise (`Chop.draw`);
      4. bandlimit's draws for its rows likewise (`BandLimit.draw`).
    Each op then runs on its own rows and the results are scattered back.  The generators of the
    member objects are not used.  In `PCMShardLoader` this is the third of four stages: whisper,
    reverb, distort, additive (`datasets._STAGES`); `Whisper` is a stage of its own, not a kind."""

    def __init__(self, kinds, seed=None):
        items = list(kinds.items()) if isinstance(kinds, dict) else [
            (getattr(k, 'kind', None), k) for k in kinds]
        self.ops = {}
        for name, obj in items:
            if name not in DISTORT_KINDS or not callable(getattr(obj, 'apply', None)):
                raise ValueError('Distort: kinds must be Clip / Chop / BandLimit objects (names '
                                 '{}), got {!r}'.format(list(DISTORT_KINDS), name))
            if name in self.ops:
                raise ValueError('Distort: {} is given twice'.format(name))
            self.ops[name] = obj
        if not self.ops:
            raise ValueError('Distort: no kind enabled')
        self.enabled = [k for k in DISTORT_KINDS if k in self.ops]
        self.rng = np.random.default_rng(seed)

    def draw_kinds(self, rng, rows):
        return rng.integers(len(self.enabled), size=rows)

    def apply(self, wave, generator=None, prev=None, lengths=None):
        """wave [B, T] (fp32 CUDA) -> (out [B, T], info).  prev (optional fp32 CUDA [B]): the
        sample preceding each row (zeros without it); lengths: host integers.  info: kinds (numpy
        array of the rows' kind names, host), prev (device [B]: what a pre-emphasis that follows
        needs — clamped by clip, untouched by chop, filtered by bandlimit), status (device int32
        [B]: the row's own op's status) and, under each kind's name that got rows, that op's info
        with `index` (numpy: its rows)."""
        ops._chk(wave, 'wave', 2)
        rows = wave.shape[0]
        rng = self.rng if generator is None else generator
        lens = None if lengths is None else np.asarray(torch.as_tensor(lengths).cpu(),
                                                       dtype=np.int64).reshape(-1)
        if lens is not None and len(lens) != rows:
            raise ValueError('Distort: lengths must hold {} integers'.format(rows))
        if prev is None:
            prev = torch.zeros(rows, device=wave.device, dtype=torch.float32)
        code = self.draw_kinds(rng, rows)
        info = dict(kinds=np.asarray(self.enabled, dtype=object)[code])
        out = prev_out = status = None
        for c, name in enumerate(self.enabled):
            idx = np.nonzero(code == c)[0]
            if len(idx) == 0:
                continue
            sub_len = None if lens is None else lens[idx]
            if len(idx) == rows:      # one kind for the whole batch: nothing to gather or scatter
                out, sub = self.ops[name].apply(wave, generator=rng, prev=prev, lengths=sub_len)
                prev_out, status = sub['prev'], sub['status']
            else:
                if out is None:
                    out, prev_out = torch.empty_like(wave), torch.empty_like(prev)
                    status = torch.empty(rows, device=wave.device, dtype=torch.int32)
                idx_d = ops._upload(torch.from_numpy(idx), wave.device)
                y, sub = self.ops[name].apply(wave.index_select(0, idx_d), generator=rng,
                                              prev=prev.index_select(0, idx_d), lengths=sub_len)
                out.index_copy_(0, idx_d, y)
                prev_out.index_copy_(0, idx_d, sub['prev'])
                status.index_copy_(0, idx_d, sub['status'])
            sub['index'] = idx
            info[name] = sub
        info.update(prev=prev_out, status=status)
        return out, info

    def __call__(self, wav):
        """Distort one waveform (numpy array or tensor, any shape: flattened)."""
        return _one_wave(self.apply, wav)


# ---------------------------------------------------------------------------------
# whispered speech.  Every default below is this project's own choice, not
# taken from a paper.
# ---------------------------------------------------------------------------------
class Whisper(_RowDistortion):
    """Pseudo-whisper by noise-excited LPC resynthesis (`ops.whisper_rows`): every frame keeps its
    spectral envelope and energy, the glottal excitation is replaced by noise.  Per row a noise
    seed and a spectral tilt tau drawn uniformly from `tilts` (each in [0, 1); 0 = white
    excitation, 0.9 lifts the excitation by nearly 6 dB per octave).  `lag_hz`: the width of the
    lag window that smooths the envelope.  Not a `Distort` kind: whisper is a property of the
    talker and runs before the room."""

    def __init__(self, tilts=(0.0, 0.5, 0.9), lag_hz=120.0, seed=None):
        self.tilts = np.asarray(list(tilts), dtype=np.float64).reshape(-1)
        if len(self.tilts) == 0 or not ((self.tilts >= 0) & (self.tilts < 1)).all():
            raise ValueError('Whisper: tilts must be non-empty and lie in [0, 1), got {}'.format(
                list(tilts)))
        ops.whisper_tables(lag_hz)      # refuses a lag_hz it cannot use
        self.lag_hz = float(lag_hz)
        self.rng = np.random.default_rng(seed)

    def draw(self, rng, rows, seeds=None, tilt_ids=None):
        """(seeds int64 [rows], tilt_ids int64 [rows]) from two vectorised draws in this order:
        the rows' noise seeds, uniform over 0 .. 2^63 - 1, then their tilt ids.  Values passed in
        are checked, kept and not drawn."""
        if seeds is None:
            seeds = rng.integers(0, 2 ** 63, size=rows, dtype=np.int64)
        else:
            seeds = np.asarray(seeds, dtype=np.int64).reshape(-1)
            if len(seeds) != rows or (seeds < 0).any():
                raise ValueError('Whisper: {} seeds in 0 .. 2^63 - 1 expected, got {}'.format(
                    rows, seeds.tolist()))
        return seeds, _draw_ids(rng, len(self.tilts), rows, tilt_ids, 'Whisper', 'tilt ids')

    def apply(self, wave, generator=None, seeds=None, tilt_ids=None, lengths=None, prev=None):
        """wave [B, T] (fp32 CUDA) -> (whispered [B, T], info).  `seeds`, `tilt_ids` (per row)
        replace the draws.  info: the dict of `ops.whisper_rows` (prev = the whispered sample
        preceding each row, status, nsilent, minorder, peak) plus seeds, tilt_ids, tilts (numpy,
        host)."""
        ops._chk(wave, 'wave', 2)
        seeds, ids = self.draw(self.rng if generator is None else generator, wave.shape[0], seeds,
                               tilt_ids)
        out, info = ops.whisper_rows(wave, seeds, self.tilts[ids], lengths, prev,
                                     lag_hz=self.lag_hz)
        info.update(seeds=seeds, tilt_ids=ids, tilts=self.tilts[ids])
        return out, info


class ComposeAdditive(object):
    """utils.py:43-49: x -> (x, additive(x))."""

    def __init__(self, additive):
        self.additive = additive

    def __call__(self, x):
        return x, self.additive(x)
