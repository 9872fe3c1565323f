"""Viterbi note decoding: per key a three-state hidden Markov model -- 0 = OFF, 1 = ONSET, 2 = SUSTAIN -- over the onset
and the frame posteriorgram, decoded by Viterbi.  The path trades the evidence of a frame against the cost of switching a note on or
off, so gap bridging and short-note removal fall out of one set of penalties.

The host functions are the definition: NumPy in int64, every value that decides the path an integer; floating point appears only
where ``NoteHMM.tables`` builds the tables.  ``viterbi_states_device`` / ``extract_notes_hmm_device`` run the same definition on the
device (csrc/hmm.hip: parallel over time, up to 16 parameter sets per call) and raise on CPU tensors -- there is no fallback.

One parameter set is ``(tables, trans)``: ``tables`` uint16 [6][256] = EO[OFF], EO[ONSET], EO[SUSTAIN], EF[OFF], EF[ONSET], EF[SUSTAIN]
(the emission cost of state s at frame t is EO[s][q(onsets[t])] + EF[s][q(frames[t])]) and ``trans`` int32 [12] = init[3], then A[3][3]
row-major with A[from][to]; an entry of ``trans`` is -1 (forbidden) or in 0..65535, and init[0] and A[0][0] must be allowed.
"""
import itertools

import numpy as np
import torch

from .decoding import _device_rolls, decode_notes

OFF, ONSET, SUSTAIN = 0, 1, 2
KEYS = 88
INF = 1 << 60                                  # "forbidden" in the int64 recurrence; sums are clamped to it
MAX_TRANS = 65535
MAX_PENALTY = 2047                             # nats: rint(32 * 2047) still fits a trans entry
COST_SCALE = 32                                # table and penalty units per nat
MAX_TABLE_COST = 4095
DEVICE_CHUNK_FRAMES = 64                       # frames per lane of the device decoder (RV_HMM_CHUNK in csrc/hmm.hip)
MAX_DEVICE_SETS = 16                           # parameter sets per rv_hmm_decode call
MAX_DEVICE_FRAMES = 1 << 20


def _roll(x):
    return np.ascontiguousarray(torch.as_tensor(x).detach().to(torch.float32).cpu().numpy())


def quantise(x):
    """q(x) as uint8, any shape: 0 unless x >= 0 (NaN and negative values), else min(255, floor(256 x)) evaluated in float32 --
    256 x is exact there, so the device arrives at the same integer.  +inf and every x >= 1 give 255."""
    x = np.asarray(x, dtype=np.float32)
    ok = x >= np.float32(0)                                             # False for NaN
    y = np.where(ok, x, np.float32(0)) * np.float32(256)
    return np.floor(np.minimum(y, np.float32(255))).astype(np.uint8)


def _check_set(tables, trans):
    """(tables as uint16 [6, 256], init int64 [3], A int64 [3, 3]) with forbidden entries at INF; ValueError on anything illegal."""
    tables = np.asarray(tables)
    if tables.shape != (6, 256) or tables.dtype.kind not in 'ui' or tables.min() < 0 or tables.max() > 65535:
        raise ValueError(f'tables must be [6, 256] integers in 0..65535, got {tables.dtype} {tables.shape}')
    trans = np.asarray(trans)
    if trans.shape != (12,) or trans.dtype.kind not in 'ui' or trans.min() < -1 or trans.max() > MAX_TRANS:
        raise ValueError(f'trans must be 12 integers, each -1 or in 0..{MAX_TRANS}, got {trans!r}')
    if trans[0] < 0 or trans[3] < 0:
        raise ValueError('init[OFF] and A[OFF][OFF] must be allowed: otherwise no path may exist')
    cost = np.where(trans < 0, INF, trans.astype(np.int64))
    return tables.astype(np.uint16), cost[:3].copy(), cost[3:].reshape(3, 3).copy()


def viterbi_states(onsets, frames, tables, trans):
    """The definition.  ``onsets`` / ``frames`` [T, 88] (arrays or tensors; they may be the same roll) -> (states uint8 [T, 88],
    cost int64 [88]).  alpha_0(s) = init[s] + E_0(s); alpha_t(s) = min_s' (alpha_{t-1}(s') + A[s'][s]) + E_t(s); bp_t(s) is the
    LOWEST s' that attains the minimum (0 when no predecessor is allowed); the last state is the lowest s that attains
    min_s alpha_{T-1}(s) = ``cost``, and the path follows bp backwards from it.  Exact in int64."""
    tables, init, A = _check_set(tables, trans)
    qo, qf = quantise(_roll(onsets)), quantise(_roll(frames))
    if qo.ndim != 2 or qo.shape[1] != KEYS or qo.shape != qf.shape or qo.shape[0] < 1:
        raise ValueError(f'expected two [T, 88] rolls with T >= 1, got {qo.shape} and {qf.shape}')
    T = qo.shape[0]
    wide = tables.astype(np.int64)
    E = wide[:3][:, qo] + wide[3:][:, qf]                               # [3, T, 88]
    alpha = np.minimum(INF, init[:, None] + E[:, 0])
    bp = np.zeros((T, 3, KEYS), np.uint8)
    for t in range(1, T):
        cand = np.minimum(INF, alpha[:, None, :] + A[:, :, None])       # [from, to, key]
        bp[t] = cand.argmin(axis=0)                                     # argmin: the first, i.e. lowest, of equal values
        alpha = np.minimum(INF, cand.min(axis=0) + E[:, t])
    cost = alpha.min(axis=0)
    s = alpha.argmin(axis=0)
    states, keys = np.zeros((T, KEYS), np.uint8), np.arange(KEYS)
    states[T - 1] = s
    for t in range(T - 1, 0, -1):
        s = bp[t, s, keys]
        states[t - 1] = s
    return states, cost.astype(np.int64)


def states_to_rolls(states):
    """(onset_roll, frame_roll) float32 0 / 1 [T, 88]: ONSET frames, and ONSET or SUSTAIN frames."""
    states = np.asarray(states)
    return (states == ONSET).astype(np.float32), (states != OFF).astype(np.float32)


class NoteHMM:
    """The model users see.  ``onset_threshold`` / ``frame_threshold`` (strictly inside (0, 1)) place the point where a roll's value
    speaks neither for nor against "on"; ``note_on`` / ``note_off`` / ``restrike`` (nats, 0..2047) are the costs of OFF -> ONSET,
    ONSET or SUSTAIN -> OFF, and SUSTAIN -> ONSET.  ``use_onsets=False`` ignores the onset roll (frame-only models, which pass the frame
    roll twice).  The three defaults of 2.0 are placeholders: no accuracy effect is claimed for them."""

    def __init__(self, onset_threshold=0.5, frame_threshold=0.5, note_on=2.0, note_off=2.0, restrike=2.0, use_onsets=True):
        for name, v in (('onset_threshold', onset_threshold), ('frame_threshold', frame_threshold)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 < float(v) < 1.0:
                raise ValueError(f'{name} must lie strictly inside (0, 1), got {v!r}')
        for name, v in (('note_on', note_on), ('note_off', note_off), ('restrike', restrike)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= float(v) <= MAX_PENALTY:
                raise ValueError(f'{name} must lie in 0..{MAX_PENALTY} nats, got {v!r}')
        if not isinstance(use_onsets, (bool, np.bool_)):
            raise ValueError(f'use_onsets must be a bool, got {use_onsets!r}')
        self.onset_threshold, self.frame_threshold = float(onset_threshold), float(frame_threshold)
        self.note_on, self.note_off, self.restrike = float(note_on), float(note_off), float(restrike)
        self.use_onsets = bool(use_onsets)

    def as_dict(self):
        return dict(onset_threshold=self.onset_threshold, frame_threshold=self.frame_threshold, note_on=self.note_on,
                    note_off=self.note_off, restrike=self.restrike, use_onsets=self.use_onsets)

    def __repr__(self):
        return 'NoteHMM(' + ', '.join(f'{k}={v!r}' for k, v in self.as_dict().items()) + ')'

    def __eq__(self, other):
        return isinstance(other, NoteHMM) and self.as_dict() == other.as_dict()

    def __hash__(self):
        return hash(tuple(self.as_dict().items()))

    @staticmethod
    def _costs(threshold):
        """(on, off) int64 [256]: for bucket q with centre c = (q + 0.5) / 256 and z = logit(c) - logit(threshold), the costs
        min(4095, rint(32 softplus(-z))) of "on" and min(4095, rint(32 softplus(z))) of "off"; float64."""
        c = (np.arange(256, dtype=np.float64) + 0.5) / 256.0
        z = np.log(c / (1.0 - c)) - np.log(threshold / (1.0 - threshold))
        on = np.minimum(MAX_TABLE_COST, np.rint(COST_SCALE * np.logaddexp(0.0, -z)))
        off = np.minimum(MAX_TABLE_COST, np.rint(COST_SCALE * np.logaddexp(0.0, z)))
        return on.astype(np.int64), off.astype(np.int64)

    def tables(self):
        """(tables uint16 [6, 256], trans int32 [12]).  EO rows are [off_o, on_o, off_o] (all zero without onsets), EF rows
        [off_f, on_f, on_f]; with a, b, c = rint(32 (note_on, note_off, restrike)): A = [[0, a, -1], [b, 0, 0], [b, c, 0]] and
        init = [0, a, -1]."""
        on_o, off_o = self._costs(self.onset_threshold)
        on_f, off_f = self._costs(self.frame_threshold)
        if not self.use_onsets:
            on_o, off_o = np.zeros(256, np.int64), np.zeros(256, np.int64)
        tables = np.stack([off_o, on_o, off_o, off_f, on_f, on_f]).astype(np.uint16)
        a, b, c = (int(np.rint(COST_SCALE * v)) for v in (self.note_on, self.note_off, self.restrike))
        trans = np.array([0, a, -1, 0, a, -1, b, 0, 0, b, c, 0], dtype=np.int32)
        return tables, trans


def _as_set(h):
    """(tables, trans) of a NoteHMM or of a raw pair."""
    return h.tables() if isinstance(h, NoteHMM) else (h[0], h[1])


def path_notes(states, velocity=None, min_frames=1, bridge_gap=0, device=False):
    """The notes of one Viterbi path, ``states`` [T, 88], as ``decoding.decode_notes`` returns them: what the threshold decoder finds at
    rule2 and 0.5 / 0.5 in the path's ONSET roll and its ONSET-or-SUSTAIN roll (``device``: torch ops on the path's device, then the device
    decoder).  A note starts where the path enters ONSET and ends at the first OFF frame; a re-strike inside a sounding note starts a
    second note that shares its end; a note's velocity is the mean of ``velocity`` over its ONSET frames."""
    on, fr = ((states == ONSET).to(torch.float32), (states != OFF).to(torch.float32)) if device else states_to_rolls(states)
    return decode_notes(on, fr, velocity, 0.5, 0.5, 'rule2', min_frames, bridge_gap, device)


def extract_notes_hmm(onsets, frames, hmm, min_frames=1, bridge_gap=0):
    """(pitches, intervals) in frame units: ``path_notes`` of the Viterbi path of ``hmm``."""
    return path_notes(viterbi_states(onsets, frames, *_as_set(hmm))[0], None, min_frames, bridge_gap)[:2]


def hmm_grid(onset_thresholds, frame_thresholds, note_on, note_off, restrike, use_onsets=True):
    """The product of the five lists as a list of ``NoteHMM``, the last list varying fastest."""
    lists = [np.atleast_1d(np.asarray(v, dtype=np.float64)).tolist() for v in (onset_thresholds, frame_thresholds, note_on, note_off, restrike)]
    return [NoteHMM(*combo, use_onsets=use_onsets) for combo in itertools.product(*lists)]


# ---------------------------------------------------------------------------------------------
# the device path (csrc/hmm.hip)
# ---------------------------------------------------------------------------------------------
def viterbi_states_device(onsets, frames, hmms):
    """``viterbi_states`` for every set of ``hmms`` (``NoteHMM`` objects or raw ``(tables, trans)`` pairs) on the rolls' device:
    (states uint8 [G, T, 88], cost int64 [G, 88]), both left on the device.  rv_hmm_decode takes 16 sets per call; longer lists run in
    batches of 16 on the same rolls.  Raises on CPU tensors: no fallback."""
    from . import _lib
    sets = []
    for h in hmms:
        tables, trans = _as_set(h)
        sets.append((_check_set(tables, trans)[0], np.asarray(trans).astype(np.int32)))       # a bad set raises here, before any launch
    if not sets:
        raise ValueError('viterbi_states_device: no parameter set')
    on, fr = _device_rolls(onsets, frames)
    T, dev, G = on.shape[0], on.device, len(sets)
    if not 1 <= T <= MAX_DEVICE_FRAMES:
        raise ValueError(f'viterbi_states_device: T = {T} not in 1..{MAX_DEVICE_FRAMES}')
    with torch.cuda.device(dev):
        states = torch.empty((G, T, KEYS), dtype=torch.uint8, device=dev)
        cost = torch.empty((G, KEYS), dtype=torch.int64, device=dev)
        ws_bytes = _lib.load().rv_hmm_workspace_bytes(T, min(G, MAX_DEVICE_SETS))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        for g0 in range(0, G, MAX_DEVICE_SETS):
            batch = sets[g0:g0 + MAX_DEVICE_SETS]
            tables = torch.from_numpy(np.stack([s[0] for s in batch]).view(np.int16)).to(dev)      # torch has no uint16 arithmetic: bits only
            trans = np.ascontiguousarray(np.stack([s[1] for s in batch]))                         # stays on the host
            _lib.call('rv_hmm_decode', on.data_ptr(), fr.data_ptr(), T, tables.data_ptr(), trans.ctypes.data, len(batch),
                      states[g0:].data_ptr(), cost[g0:].data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream())
    return states, cost


def extract_notes_hmm_device(onsets, frames, hmms, min_frames=1, bridge_gap=0):
    """``extract_notes_hmm`` for every set of ``hmms`` on the device: one batched Viterbi decode per 16 sets, then per set ``path_notes``
    (rv_eval_decode_clean on the path's two 0 / 1 rolls).  Returns one (pitches, intervals, painted) per set, as
    ``extract_notes_wo_velocity_device`` does."""
    states, _ = viterbi_states_device(onsets, frames, hmms)
    return [(p, i, painted) for p, i, _, painted in (path_notes(s, None, min_frames, bridge_gap, True) for s in states)]
