"""Note decoding of the posteriorgrams (evaluation / inference path).

Same results as the reference's ``model/decoding.py`` (pinned by tests/golden/decoding.npz, produced by running the
reference functions), computed without the reference's per-note Python ``while`` loop: the end of every note is a
lookup in a per-pitch "next inactive frame" table built with one reverse cumulative minimum.

``NoteDecoder`` is the one answer to "how do two posteriorgrams become notes" -- threshold or HMM, host or device, with or without a
velocity roll and the clean-up; the ``extract_notes_*`` functions are its building blocks and keep their results.
"""
import numpy as np
import torch


def _binarise(onsets, frames, onset_threshold, frame_threshold):
    on = (torch.as_tensor(onsets) > onset_threshold).cpu().numpy()
    fr = (torch.as_tensor(frames) > frame_threshold).cpu().numpy()
    return on, fr


def _note_ends(active):
    """next_off[t, p] = smallest t' >= t with active[t', p] == False (T if none)."""
    T = active.shape[0]
    idx = np.where(~active, np.arange(T)[:, None], T)
    return np.minimum.accumulate(idx[::-1], axis=0)[::-1]


MAX_MIN_FRAMES, MAX_BRIDGE_GAP = 32, 31         # the look-ahead / look-back of the device decoder stays inside one 64-frame tile


def _cleanup_args(min_frames, bridge_gap):
    """(min_frames, bridge_gap) as ints; ValueError unless they are integers in 1..32 and 0..31."""
    for name, v, lo, hi in (('min_frames', min_frames, 1, MAX_MIN_FRAMES), ('bridge_gap', bridge_gap, 0, MAX_BRIDGE_GAP)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f'{name} must be an integer in {lo}..{hi}, got {v!r}')
    return int(min_frames), int(bridge_gap)


def _bridge_gaps(active, gap):
    """``active`` [T, P] with every maximal inactive run of at most ``gap`` frames switched on, if it has an active frame directly
    before it and directly after it (a run that touches frame 0 or frame T - 1 has not)."""
    T = active.shape[0]
    t = np.arange(T)[:, None]
    before = np.maximum.accumulate(np.where(active, t, -1), axis=0)                     # last active frame <= t (-1 if none)
    after = np.minimum.accumulate(np.where(active, t, T)[::-1], axis=0)[::-1]           # first active frame >= t (T if none)
    return active | ((before >= 0) & (after < T) & (after - before - 1 <= gap))


def extract_notes_wo_velocity(onsets, frames, onset_threshold=0.5, frame_threshold=0.5, rule='rule1', min_frames=1, bridge_gap=0):
    """model/decoding.py:4-56.  A note starts where the thresholded onset roll rises (rule1: and the frame roll is on)
    and lasts while the onset OR the frame roll stays on.  Returns (pitches [N], intervals [N, 2]) in frame units,
    ordered by (onset frame, pitch) like the reference.

    Note clean-up (``min_frames=1, bridge_gap=0`` is the reference's decoder): ``bridge_gap`` = g, 0..31, switches on,
    per pitch, every inactive run of the onset-OR-frame activity that is at most g frames long and lies between two active frames
    -- the starts (and rule1's test of the frame roll) are those of the unbridged rolls; ``min_frames`` = m, 1..32, drops the notes
    that end less than m frames after their start in the bridged activity."""
    if rule not in ('rule1', 'rule2'):
        raise NameError('Please enter the correct rule name')
    min_frames, bridge_gap = _cleanup_args(min_frames, bridge_gap)
    on, fr = _binarise(onsets, frames, onset_threshold, frame_threshold)
    onset_diff = np.concatenate([on[:1], on[1:] & ~on[:-1]], axis=0)
    if rule == 'rule1':
        onset_diff = onset_diff & fr
    t, p = np.nonzero(onset_diff)
    active = on | fr
    if bridge_gap:
        active = _bridge_gaps(active, bridge_gap)
    ends = _note_ends(active)[t, p]
    keep = ends - t >= min_frames
    pitches = p[keep]
    intervals = np.stack([t[keep], ends[keep]], axis=1) if keep.any() else np.array([])
    return (pitches if keep.any() else np.array([])), intervals


def extract_notes(onsets, frames, velocity, onset_threshold=0.5, frame_threshold=0.5):
    """model/decoding.py:59-107: as above without the frame condition, plus the mean velocity over the note's
    onset-active frames."""
    on, fr = _binarise(onsets, frames, onset_threshold, frame_threshold)
    vel = torch.as_tensor(velocity).cpu().numpy()
    onset_diff = np.concatenate([on[:1], on[1:] & ~on[:-1]], axis=0)
    t, p = np.nonzero(onset_diff)
    ends = _note_ends(on | fr)[t, p]
    pitches, intervals, velocities = [], [], []
    for a, b, q in zip(t, ends, p):
        if b > a:
            m = on[a:b, q]
            pitches.append(q)
            intervals.append([a, b])
            velocities.append(float(np.mean(vel[a:b, q][m])) if m.any() else 0)
    return np.array(pitches), np.array(intervals), np.array(velocities)


def notes_to_frames(pitches, intervals, shape):
    """model/decoding.py:109-130: piano roll of the notes -> (frame indices, list of active-bin arrays)."""
    roll = np.zeros(tuple(shape))
    for pitch, (onset, offset) in zip(pitches, intervals):
        roll[onset:offset, pitch] = 1
    time = np.arange(roll.shape[0])
    freqs = [roll[t, :].nonzero()[0] for t in time]
    return time, freqs


def note_velocities(onsets, velocity, onset_threshold, pitches, intervals):
    """float32 [n]: per note (pitch, [t, end)) the mean of velocity[s, pitch] over t <= s < end with onsets[s, pitch] >
    onset_threshold -- summed in float64 in ascending s, divided in float64, rounded to float32 once; 0 if no such frame exists.
    The arithmetic of rv_eval_note_velocity (csrc/velocity.hip), bit for bit."""
    on = (torch.as_tensor(onsets) > onset_threshold).cpu().numpy()
    vel = torch.as_tensor(velocity).detach().to(torch.float32).cpu().numpy()
    out = np.zeros(len(pitches), dtype=np.float32)
    for i, (p, (a, b)) in enumerate(zip(pitches, np.asarray(intervals).reshape(-1, 2))):
        p, a, b = int(p), int(a), min(int(b), on.shape[0])
        v = vel[a:b, p][on[a:b, p]].astype(np.float64)
        if v.size:
            out[i] = np.float32(np.add.accumulate(v)[-1] / np.float64(v.size))      # accumulate: strictly left to right
    return out


def extract_notes_with_velocity(onsets, frames, velocity, onset_threshold=0.5, frame_threshold=0.5, rule='rule2', min_frames=1,
                                bridge_gap=0):
    """``extract_notes_wo_velocity`` plus ``note_velocities`` of its notes: (pitches, intervals, velocities).  At rule2 / (1, 0) these
    are the notes of the reference's ``extract_notes`` with its velocities (there a float32 mean)."""
    pitches, intervals = extract_notes_wo_velocity(onsets, frames, onset_threshold, frame_threshold, rule=rule, min_frames=min_frames,
                                                   bridge_gap=bridge_gap)
    return pitches, intervals, note_velocities(onsets, velocity, onset_threshold, pitches, intervals)


# ---------------------------------------------------------------------------------------------
# the device path (csrc/eval.hip, csrc/velocity.hip)
# ---------------------------------------------------------------------------------------------
_RULES = {'rule1': 1, 'rule2': 2}
DEVICE_TILE_FRAMES = 64                        # frames per workgroup of the device decoder (RV_EVAL_TILE in csrc/eval.hip)


def _device_rolls(*rolls):
    """The rolls as the kernels load them: float32, contiguous, 16-byte aligned.  RuntimeError on a CPU tensor (no fallback), ValueError
    unless they are [T, 88] rolls of one shape on one device."""
    from . import _lib
    _lib.need_gpu(*rolls)
    out = [x.detach().to(torch.float32).contiguous() for x in rolls]
    out = [x.clone() if x.data_ptr() % 16 else x for x in out]
    if any(x.dim() != 2 or x.shape[1] != 88 or x.shape != out[0].shape or x.device != out[0].device for x in out):
        raise ValueError(f'expected [T, 88] rolls of one song on one device, got {[tuple(x.shape) for x in out]}')
    return out


def extract_notes_device(onsets, frames, velocity, onset_threshold=0.5, frame_threshold=0.5, rule='rule2', min_frames=1, bridge_gap=0):
    """``extract_notes_with_velocity`` on the device: the rolls stay in HBM, rv_eval_decode_clean decodes them in
    three launches, and the only read-back is the note count followed by that many (t, pitch, end) rows; from the rows while they are
    still in HBM, rv_eval_note_velocity.  Returns (pitches, intervals, velocities float32 [n], painted): pitches / intervals are NumPy
    arrays equal to the host function's; painted is the uint8 [T, 88] roll of the notes -- what ``notes_to_frames`` paints -- left on
    the device for ``evaluate.evaluate_frames_device``.  ``velocity=None``: no velocity launch, velocities None."""
    from . import _lib
    if rule not in _RULES:
        raise NameError('Please enter the correct rule name')
    min_frames, bridge_gap = _cleanup_args(min_frames, bridge_gap)
    on, fr, *vel = _device_rolls(onsets, frames, *(() if velocity is None else (velocity,)))
    T, dev = on.shape[0], on.device
    max_notes = 88 * ((T + 1) // 2)                    # a pitch cannot rise more often than every other frame
    with torch.cuda.device(dev):
        ws_bytes = _lib.load().rv_eval_workspace_bytes(T)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        notes = torch.empty((max(max_notes, 1), 3), dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        painted = torch.empty((T, 88), dtype=torch.uint8, device=dev)
        _lib.call('rv_eval_decode_clean', on.data_ptr(), fr.data_ptr(), T, float(onset_threshold), float(frame_threshold), _RULES[rule],
                  min_frames, bridge_gap, notes.data_ptr(), max_notes, count.data_ptr(), painted.data_ptr(), ws.data_ptr(), ws_bytes,
                  _lib.stream())
        n = int(count.item())
        if n > max_notes:
            raise RuntimeError(f'rv_eval_decode_clean reported {n} notes, more than the bound of {max_notes}')
        velocities = None
        if vel:
            out = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
            _lib.call('rv_eval_note_velocity', on.data_ptr(), vel[0].data_ptr(), T, float(onset_threshold), notes.data_ptr(), n,
                      out.data_ptr(), out.numel(), _lib.stream())
            velocities = out[:n].cpu().numpy()
    if n == 0:
        return np.array([]), np.array([]), velocities, painted
    rows = notes[:n].cpu().numpy().astype(np.int64)
    return rows[:, 1].copy(), np.ascontiguousarray(rows[:, [0, 2]]), velocities, painted


def extract_notes_wo_velocity_device(onsets, frames, onset_threshold=0.5, frame_threshold=0.5, rule='rule1', min_frames=1, bridge_gap=0):
    """``extract_notes_wo_velocity`` on the device: (pitches, intervals, painted) of ``extract_notes_device`` without a velocity roll."""
    pitches, intervals, _, painted = extract_notes_device(onsets, frames, None, onset_threshold, frame_threshold, rule, min_frames, bridge_gap)
    return pitches, intervals, painted


# ---------------------------------------------------------------------------------------------
# the one decoder
# ---------------------------------------------------------------------------------------------
def decode_notes(onsets, frames, velocity=None, onset_threshold=0.5, frame_threshold=0.5, rule='rule1', min_frames=1, bridge_gap=0,
                 device=False):
    """The threshold decode on either side: (pitches, intervals, velocities or None, painted or None).  ``device=False`` runs the host
    functions -- on tensors of any device -- and paints nothing; ``device=True`` is ``extract_notes_device``."""
    if device:
        return extract_notes_device(onsets, frames, velocity, onset_threshold, frame_threshold, rule, min_frames, bridge_gap)
    pitches, intervals = extract_notes_wo_velocity(onsets, frames, onset_threshold, frame_threshold, rule, min_frames, bridge_gap)
    velocities = None if velocity is None else note_velocities(onsets, velocity, onset_threshold, pitches, intervals)
    return pitches, intervals, velocities, None


class NoteDecoder:
    """How two posteriorgrams become notes.  Built once from what the callers pass -- the two thresholds, ``rule``, the clean-up
    (``min_frames`` / ``bridge_gap``) and optionally ``hmm``, a ``hmm.NoteHMM`` -- and every argument error
    is raised here, before any song is touched: NameError for the rule, ValueError for the clean-up, TypeError for an ``hmm`` of
    another type, ValueError for a model that uses onsets where the caller decodes the frame roll alone (``onset=False``).

    ``decoder(onsets, frames, velocity=None, device=False)`` -> (pitches, intervals, velocities or None, painted or None) as
    ``decode_notes`` returns them.  With a model the notes are those of its Viterbi path (``hmm.path_notes``): the two thresholds and
    the rule are unused, the clean-up applies, and a note's velocity is the mean over the path's ONSET frames.  ``device`` is the
    caller's choice, never derived from the tensors: the host functions take device tensors too.  A new way of decoding belongs here."""

    def __init__(self, onset_threshold=0.5, frame_threshold=0.5, rule='rule1', min_frames=1, bridge_gap=0, hmm=None, onset=True):
        if rule not in _RULES:
            raise NameError('Please enter the correct rule name')
        self.min_frames, self.bridge_gap = _cleanup_args(min_frames, bridge_gap)
        if hmm is not None:
            from .hmm import NoteHMM
            if not isinstance(hmm, NoteHMM):
                raise TypeError(f'hmm must be a NoteHMM, got {type(hmm).__name__}')
            if not onset and hmm.use_onsets:
                raise ValueError('onset=False decodes the frame roll alone: the NoteHMM must have use_onsets=False')
        self.onset_threshold, self.frame_threshold, self.rule, self.hmm = onset_threshold, frame_threshold, rule, hmm

    def __call__(self, onsets, frames, velocity=None, device=False):
        if self.hmm is None:
            return decode_notes(onsets, frames, velocity, self.onset_threshold, self.frame_threshold, self.rule, self.min_frames,
                                self.bridge_gap, device)
        from . import hmm as nh
        if device:
            states = nh.viterbi_states_device(onsets, frames, [self.hmm])[0][0]
        else:
            states = nh.viterbi_states(onsets, frames, *self.hmm.tables())[0]
        return nh.path_notes(states, velocity, self.min_frames, self.bridge_gap, device)
