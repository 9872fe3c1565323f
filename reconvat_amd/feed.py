"""Device-side data feed: the corpus stays in HBM as int16 audio / uint8 rolls and every batch is
cropped and decoded by ONE pair of kernel launches (rv_crop_segments) instead of per-item host slicing, float
conversion and host->device copies.

``DeviceCorpus`` takes the tracks of a ``PianoRollAudioDataset`` (reference model/dataset.py:19-142 contract) and
reproduces ``DataLoader(dataset, batch_size, shuffle=True, drop_last=True)`` + ``__getitem__`` semantics:
  * item order: a fresh ``torch.randperm`` per epoch (the DataLoader's RandomSampler);
  * crop position of every item: ``RandomState(seed).randint(T - L) // 512`` drawn in item order
    (model/dataset.py:41) -- bit-identical batches to the host path for the same seeds (tests/test_feed_gpu.py);
  * with ``world > 1`` rank r keeps tracks r, r + world, ... (per-rank shard, disjoint data on every GPU).
A 8 x 327 680-sample batch is 5 MB of int16 in, 10 MB of fp32 + 9 MB of label masks out: ~10 us of HBM streaming.
There is no CPU fallback: the corpus tensors must live on a HIP device.

``pitch_shift=p`` (off by default; DESIGN 3.12, reconvat_amd/augment.py) makes every item a copy of its crop transposed by a random
whole number of semitones in [-p, p]: ``rv_crop_segments_shift`` resamples the audio while it crops and moves the labels along.

``acoustics=Acoustics(...)`` (off by default; DESIGN 3.14, reconvat_amd/acoustics.py) records every item in another room, through another
microphone and over a noise floor: the crop, shifted or plain, goes to a scratch buffer and ``rv_fir_items`` filters it with the
item's own FIR into the batch.  The labels, the crop stream and the pitch-shift stream are untouched.
"""
import numpy as np
import torch

from . import acoustics as acu
from . import augment
from .constants import HOP_LENGTH
from ._lib import call, ptr, stream, need_gpu

ITEM_FIELDS = 12          # longs per item of rv_crop_segments_shift's table (RV_SHIFT_FIELDS in csrc/data.hip)


def _pad_to(n, m):
    return (n + m - 1) // m * m


class DeviceCorpus:
    def __init__(self, tracks, sequence_length, batch_size, device, seed=42, rank=0, world=1, sampler_seed=0, pitch_shift=0,
                 aug_seed=0, acoustics=None, acoustics_seed=0):
        tracks = list(tracks)[rank::world]
        self.pitch_shift = augment.check_shift(pitch_shift)
        if acoustics is not None and not isinstance(acoustics, acu.Acoustics):
            raise ValueError(f'acoustics must be None or an Acoustics object (got {acoustics!r})')
        self.acoustics = None if acoustics is None or acoustics.off else acoustics
        if not tracks:
            raise ValueError('DeviceCorpus: no tracks for this rank')
        self.sequence_length = int(sequence_length)
        if self.sequence_length % HOP_LENGTH:
            raise ValueError('sequence_length must be a multiple of HOP_LENGTH (512)')
        self.batch_size = int(batch_size)
        self.device = torch.device(device)
        self.n_keys = int(tracks[0]['label'].shape[1])
        self.paths = [t['path'] for t in tracks]
        self.lengths = np.array([len(t['audio']) for t in tracks], dtype=np.int64)
        if len(tracks) < self.batch_size:
            # an epoch of zero batches would make cycle(loader) spin forever
            raise ValueError(f'DeviceCorpus: rank {rank} of {world} holds {len(tracks)} track(s), fewer than batch_size='
                             f'{self.batch_size}; lower the batch size or the number of ranks')
        if (self.lengths <= self.sequence_length).any():
            raise ValueError('every track must be longer than sequence_length (the reference draws randint(T - L))')
        if self.pitch_shift:
            widest = augment.span(self.pitch_shift, self.sequence_length)
            if (self.lengths <= widest).any():
                raise ValueError(f'pitch_shift={self.pitch_shift}: every track must be longer than the {widest} samples a crop shifted up '
                                 f'by {self.pitch_shift} semitones reads (the shortest has {int(self.lengths.min())})')
        # concatenate; track starts padded to 8 samples / 16 label bytes so that aligned crops use 16-byte accesses
        a_off, l_off, na, nl = [], [], 0, 0
        for t in tracks:
            a_off.append(na)
            l_off.append(nl)
            na += _pad_to(len(t['audio']), 8)
            nl += _pad_to(t['label'].shape[0] * self.n_keys, 16)
        audio = torch.zeros(na, dtype=torch.int16)
        label = torch.zeros(nl, dtype=torch.uint8)
        velocity = torch.zeros(nl, dtype=torch.uint8)
        for t, ao, lo in zip(tracks, a_off, l_off):
            a = torch.as_tensor(t['audio'])
            audio[ao:ao + a.numel()] = a
            lab = torch.as_tensor(t['label']).reshape(-1)
            label[lo:lo + lab.numel()] = lab
            vel = torch.as_tensor(t['velocity']).reshape(-1)
            velocity[lo:lo + vel.numel()] = vel.to(torch.uint8)
        self.audio, self.label, self.velocity = audio.to(self.device), label.to(self.device), velocity.to(self.device)
        need_gpu(self.audio)
        self.a_off = np.array(a_off, dtype=np.int64)
        self.l_off = np.array(l_off, dtype=np.int64)
        self.random = np.random.RandomState(seed)                  # the reference's crop stream (one draw per item)
        self.sampler = torch.Generator().manual_seed(sampler_seed)  # item order (RandomSampler analogue)
        # crop offsets travel through a ring of pinned staging buffers, each guarded by the event of its last upload:
        # a batch drawn while an earlier upload is still queued never overwrites offsets the device has not read yet
        # (with pitch_shift the ring carries the per-item table of rv_crop_segments_shift instead)
        ring_shape = (self.batch_size, ITEM_FIELDS) if self.pitch_shift else (2, self.batch_size)
        self._ring = [torch.empty(ring_shape, dtype=torch.int64).pin_memory() for _ in range(4)]
        self._ring_events = [None] * len(self._ring)
        self._ring_pos = 0
        if self.pitch_shift:
            # a second stream for the shifts, and the 13 polyphase banks, concatenated (each starts at a multiple of 4 floats)
            self.aug = np.random.RandomState(aug_seed)
            self.n_rows = np.array([t['label'].shape[0] for t in tracks], dtype=np.int64)
            self._banks, parts, at = {}, [], 0
            for k in range(-augment.MAX_SHIFT, augment.MAX_SHIFT + 1):
                L, M, F, Kp, bank = augment.bank32(k)
                self._banks[k] = (L, M, F, Kp, at)
                parts.append(bank.reshape(-1))
                at += bank.size                                    # Kp is a multiple of 4
            self.banks = torch.from_numpy(np.concatenate(parts)).to(self.device)
        if self.acoustics is not None:
            # a third stream for the acoustic parameters; the filters of a batch, then its noise seeds and amplitudes, travel through
            # a pinned ring of their own: float32 [B W | B | B], the seeds as their bit patterns
            self.acu = np.random.RandomState(acoustics_seed)
            floats = self.batch_size * (self.acoustics.width + 2)
            self._fir_ring = [torch.empty(floats, dtype=torch.float32).pin_memory() for _ in range(4)]
            self._fir_events = [None] * len(self._fir_ring)
            self._fir_pos = 0

    def __len__(self):
        return len(self.paths) // self.batch_size                  # batches per epoch (drop_last=True)

    def draw(self, indices):
        """Crop positions and shifts for the given items, in order (model/dataset.py:41,48; augment.draw_items):
        (step_begin [B], begin [B], shift [B]).  Without pitch_shift the crop stream is used exactly as before and shift is 0."""
        steps, shifts = augment.draw_items(self.random, self.aug if self.pitch_shift else None, self.lengths, indices,
                                           self.sequence_length, self.pitch_shift)
        return steps, steps * HOP_LENGTH, shifts

    def _upload(self, fill, fir=False):
        """The next pinned staging buffer (of the filter ring with `fir`), filled by `fill(staging)`, on its way to the device."""
        ring, events = (self._fir_ring, self._fir_events) if fir else (self._ring, self._ring_events)
        slot = self._fir_pos if fir else self._ring_pos
        if fir:
            self._fir_pos = (slot + 1) % len(ring)
        else:
            self._ring_pos = (slot + 1) % len(ring)
        if events[slot] is not None:
            events[slot].synchronize()
        staging = ring[slot]
        dev = fill(staging).to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        events[slot] = ev
        return dev

    def filters(self, params):
        """float32 [b, W] filters, uint32 [b] noise seeds and float32 [b] noise amplitudes of the given parameter dicts."""
        W = self.acoustics.width
        h = np.zeros((len(params), W), dtype=np.float32)
        for i, p in enumerate(params):
            if int(p['taps']) != self.acoustics.taps:
                raise ValueError(f"crop: acoustic parameters of {p['taps']} taps, the corpus was built for {self.acoustics.taps}")
            h[i], lead = acu.item_filter(p)
            assert lead == acu.LEAD
        seeds = np.array([int(p['seed']) for p in params], dtype=np.uint32)
        amps = np.array([p['amp'] for p in params], dtype=np.float32)
        return h, seeds, amps

    def crop(self, indices, steps, shifts=None, acoustics=None):
        """The batch of the given items cropped at source rows `steps` (any row of the track), transposed by `shifts` semitones
        (None: no shift) and recorded with the per-item parameter dicts `acoustics` (acoustics.draw; None: as cropped); what batch()
        calls with what it drew."""
        indices = [int(i) for i in indices]
        b = len(indices)
        if b < 1 or b > self.batch_size:
            raise ValueError(f'crop: {b} items, expected 1..{self.batch_size}')
        steps = np.asarray(steps, dtype=np.int64).reshape(-1)
        shifts = np.zeros(b, dtype=np.int64) if shifts is None else np.asarray(shifts, dtype=np.int64).reshape(-1)
        if len(steps) != b or len(shifts) != b:
            raise ValueError('crop: one step and one shift per item')
        begins = steps * HOP_LENGTH
        n_steps = self.sequence_length // HOP_LENGTH
        if acoustics is not None:
            if self.acoustics is None:
                raise ValueError('crop: acoustic parameters need DeviceCorpus(acoustics=Acoustics(...)) with something switched on')
            acoustics = list(acoustics)
            if len(acoustics) != b:
                raise ValueError('crop: one set of acoustic parameters per item')
            fir_h, fir_seed, fir_amp = self.filters(acoustics)
        audio = torch.empty((b, self.sequence_length), device=self.device, dtype=torch.float32)
        # with acoustics the crop lands in `audio` as a scratch buffer and rv_fir_items writes the batch's audio from it
        out = {'audio': audio}
        for k in ('onset', 'offset', 'frame', 'velocity'):
            out[k] = torch.empty((b, n_steps, self.n_keys), device=self.device, dtype=torch.float32)
        if not self.pitch_shift:
            if shifts.any():
                raise ValueError('crop: shifts need DeviceCorpus(pitch_shift > 0)')
            if (steps < 0).any() or (begins + self.sequence_length > self.lengths[indices]).any():
                raise ValueError('crop: a crop does not lie inside its track')

            def fill(staging):
                staging[0, :b] = torch.from_numpy(self.a_off[indices] + begins)
                staging[1, :b] = torch.from_numpy(self.l_off[indices] + steps * self.n_keys)
                return staging[:, :b]
            dev_begins = self._upload(fill)
            call('rv_crop_segments', ptr(self.audio), ptr(self.label), ptr(self.velocity), ptr(dev_begins[0]), ptr(dev_begins[1]),
                 b, self.sequence_length, n_steps, self.n_keys, ptr(out['audio']), ptr(out['onset']), ptr(out['offset']),
                 ptr(out['frame']), ptr(out['velocity']), stream())
        else:
            if (np.abs(shifts) > augment.MAX_SHIFT).any():
                raise ValueError(f'crop: shifts must lie in -{augment.MAX_SHIFT}..{augment.MAX_SHIFT}')
            if (steps < 0).any() or (steps >= self.n_rows[indices]).any():
                raise ValueError('crop: a crop does not start inside its track')
            table = np.zeros((b, ITEM_FIELDS), dtype=np.int64)
            table[:, 0] = self.a_off[indices] + begins
            table[:, 1] = self.a_off[indices]
            table[:, 2] = self.a_off[indices] + self.lengths[indices]
            table[:, 3:8] = [self._banks[int(k)] for k in shifts]
            table[:, 8] = self.l_off[indices] + steps * self.n_keys
            table[:, 9] = self.n_rows[indices] - steps
            table[:, 10] = shifts

            def fill(staging):
                staging[:b] = torch.from_numpy(table)
                return staging[:b]
            items = self._upload(fill)
            call('rv_crop_segments_shift', ptr(self.audio), self.audio.numel(), ptr(self.label), ptr(self.velocity), self.label.numel(),
                 ptr(self.banks), self.banks.numel(), ptr(items), b, self.sequence_length, n_steps, self.n_keys, ptr(out['audio']),
                 ptr(out['onset']), ptr(out['offset']), ptr(out['frame']), ptr(out['velocity']), stream())
        if acoustics is not None:
            W = self.acoustics.width

            def fill_fir(staging):
                staging[:b * W] = torch.from_numpy(fir_h.reshape(-1))
                staging[b * W:b * W + b] = torch.from_numpy(fir_seed.view(np.float32))
                staging[b * W + b:b * W + 2 * b] = torch.from_numpy(fir_amp)
                return staging[:b * (W + 2)]
            fir = self._upload(fill_fir, fir=True)
            out['audio'] = torch.empty_like(audio)
            call('rv_fir_items', ptr(audio), self.sequence_length, ptr(fir), W, acu.LEAD, ptr(fir) + 4 * b * W, ptr(fir) + 4 * (b * W + b),
                 b, self.sequence_length, ptr(out['audio']), self.sequence_length, stream())
            out['acoustics'] = acoustics
        out['shift'] = torch.from_numpy(shifts.copy())
        out['path'] = [self.paths[i] for i in indices]
        out['start_idx'] = torch.from_numpy(begins)
        return out

    def batch(self, indices):
        """One decoded batch on the device for the given track indices (len == batch_size)."""
        indices = [int(i) for i in indices]
        steps, _, shifts = self.draw(indices)
        drawn = [acu.draw(self.acu, self.acoustics) for _ in indices] if self.acoustics is not None else None
        return self.crop(indices, steps, shifts, drawn)

    def __iter__(self):
        """One epoch: a random permutation of the tracks in batches of batch_size, last partial batch dropped."""
        perm = torch.randperm(len(self.paths), generator=self.sampler).tolist()
        for i in range(0, len(perm) - self.batch_size + 1, self.batch_size):
            yield self.batch(perm[i:i + self.batch_size])


def device_loader(dataset, batch_size, device, rank=0, world=1, seed=42, pitch_shift=0, acoustics=None):
    """DeviceCorpus over the in-memory tracks of a PianoRollAudioDataset (``dataset.data``); with world > 1 every rank
    keeps a disjoint shard (tracks rank, rank + world, ...) and its own item-order stream -- and, with ``pitch_shift``, its own
    stream of shifts and, with ``acoustics``, its own stream of acoustic parameters (both seeded from the rank's crop seed)."""
    return DeviceCorpus(dataset.data, dataset.sequence_length, batch_size, device, seed=seed, rank=rank, world=world,
                        sampler_seed=rank, pitch_shift=pitch_shift, aug_seed=1000003 + seed, acoustics=acoustics,
                        acoustics_seed=2000003 + seed)
