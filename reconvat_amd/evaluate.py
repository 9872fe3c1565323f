"""Evaluation path: ``evaluate_wo_velocity`` with the reference's metric keys
(model/evaluate_functions.py:20-127).

The reference delegates the metrics to ``mir_eval`` (multipitch.evaluate, transcription.precision_recall_f1_overlap),
which is neither vendored in the reference nor installed here.  They are restated below from their published
definitions -- PARITY UNPINNED for these two functions (no reference output available to pin them); their call sites,
argument conventions and the metric keys follow the reference, and tests/test_decoding.py checks them on cases with
known answers.  ``average_precision_score`` is scikit-learn's, as in the reference.
"""
import os
import sys
from collections import defaultdict, namedtuple

import numpy as np
import torch
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching
from scipy.stats import hmean

from . import _lib
from .constants import HOP_LENGTH, SAMPLE_RATE, MIN_MIDI
from .decoding import (_RULES, NoteDecoder, _cleanup_args, _device_rolls, extract_notes_wo_velocity, extract_notes_wo_velocity_device,
                       notes_to_frames)
from .hmm import NoteHMM, path_notes, viterbi_states, viterbi_states_device
from .midi import save_midi

eps = sys.float_info.epsilon
N_DECIMALS = 4          # mir_eval rounds time differences to 0.1 ms before comparing with a tolerance


def midi_to_hz(midi):
    return 440.0 * (2.0 ** ((np.asarray(midi, dtype=np.float64) - 69.0) / 12.0))


def _hz_to_midi(hz):
    return 12.0 * (np.log2(np.asarray(hz, dtype=np.float64)) - np.log2(440.0)) + 69.0


# ---------------------------------------------------------------------------------------------
# frame metrics (mir_eval.multipitch.evaluate: Poliner & Ellis 2007 error decomposition)
# ---------------------------------------------------------------------------------------------
def _count_matches(ref_midi, est_midi, window=0.5):
    """Maximum number of one-to-one pairs with |ref - est| < window semitones (greedy on sorted lists is optimal in 1-D)."""
    r, e = np.sort(ref_midi), np.sort(est_midi)
    i = j = n = 0
    while i < len(r) and j < len(e):
        d = r[i] - e[j]
        if abs(d) < window:
            n += 1; i += 1; j += 1
        elif d < 0:
            i += 1
        else:
            j += 1
    return n


def evaluate_frames(ref_time, ref_freqs, est_time, est_freqs, window=0.5):
    """Frame-level Precision / Recall / Accuracy and the substitution / miss / false-alarm / total errors, plus their
    chroma (octave-folded) variants.  Both sequences must be on the same time base (they are: same hop)."""
    ref_time, est_time = np.asarray(ref_time, dtype=np.float64), np.asarray(est_time, dtype=np.float64)
    if len(ref_time) != len(est_time) or not np.allclose(ref_time, est_time):
        raise ValueError('evaluate_frames: reference and estimate must share one time base')
    counts = []
    for chroma in (False, True):
        tp = n_ref = n_est = sub = miss = fa = tot = 0
        for rf, ef in zip(ref_freqs, est_freqs):
            rm = _hz_to_midi(rf) if len(rf) else np.array([])
            em = _hz_to_midi(ef) if len(ef) else np.array([])
            if chroma:
                rm, em = np.mod(rm, 12), np.mod(em, 12)
                # circular distance: try both unwrapped copies
                c = max(_count_matches(rm, em, window), _count_matches(rm, np.concatenate([em, em + 12, em - 12]), window)
                        if len(em) else 0)
                c = min(c, len(rm), len(em))
            else:
                c = _count_matches(rm, em, window)
            nr, ne = len(rm), len(em)
            tp += c; n_ref += nr; n_est += ne
            sub += min(nr, ne) - c
            miss += max(0, nr - ne)
            fa += max(0, ne - nr)
            tot += max(nr, ne) - c
        counts += [tp, n_ref, n_est, sub, miss, fa, tot]
    return _frame_metrics_from_counts(counts)


# ---------------------------------------------------------------------------------------------
# note metrics (mir_eval.transcription.precision_recall_f1_overlap)
# ---------------------------------------------------------------------------------------------
def match_notes(ref_intervals, ref_pitches, est_intervals, est_pitches, onset_tolerance=0.05, pitch_tolerance=50.0,
                offset_ratio=0.2, offset_min_tolerance=0.05):
    """Maximum one-to-one matching of notes that agree in onset (+-50 ms), pitch (+-50 cents) and -- unless
    offset_ratio is None -- offset (+-max(20 % of the reference duration, 50 ms)).  Returns [(ref_i, est_j), ...]."""
    ref_intervals = np.asarray(ref_intervals, dtype=np.float64).reshape(-1, 2)
    est_intervals = np.asarray(est_intervals, dtype=np.float64).reshape(-1, 2)
    if len(ref_intervals) == 0 or len(est_intervals) == 0:
        return []
    onset_d = np.around(np.abs(np.subtract.outer(ref_intervals[:, 0], est_intervals[:, 0])), N_DECIMALS)
    hit = onset_d <= onset_tolerance
    pitch_d = np.abs(1200.0 * np.subtract.outer(np.log2(ref_pitches), np.log2(est_pitches)))
    hit &= pitch_d <= pitch_tolerance
    if offset_ratio is not None:
        offset_d = np.around(np.abs(np.subtract.outer(ref_intervals[:, 1], est_intervals[:, 1])), N_DECIMALS)
        tol = offset_ratio * (ref_intervals[:, 1] - ref_intervals[:, 0])
        tol[tol <= offset_min_tolerance] = offset_min_tolerance
        hit &= offset_d <= tol.reshape(-1, 1)
    match = maximum_bipartite_matching(csr_matrix(hit), perm_type='column')
    return [(i, int(j)) for i, j in enumerate(match) if j >= 0]


def evaluate_notes(ref_intervals, ref_pitches, est_intervals, est_pitches, onset_tolerance=0.05, pitch_tolerance=50.0,
                   offset_ratio=0.2, offset_min_tolerance=0.05, beta=1.0, match=None):
    """(precision, recall, f-measure, average overlap ratio of the matched pairs).  ``match``: the matcher, ``match_notes`` unless
    given (``match_notes_sparse`` returns the same pairs without the dense matrices)."""
    ref_intervals = np.asarray(ref_intervals, dtype=np.float64).reshape(-1, 2)
    est_intervals = np.asarray(est_intervals, dtype=np.float64).reshape(-1, 2)
    if len(ref_pitches) == 0 or len(est_pitches) == 0:
        return 0.0, 0.0, 0.0, 0.0
    m = (match or match_notes)(ref_intervals, ref_pitches, est_intervals, est_pitches, onset_tolerance, pitch_tolerance, offset_ratio,
                               offset_min_tolerance)
    return _scores_of_matching(m, ref_intervals, est_intervals, beta)


def _scores_of_matching(m, ref_intervals, est_intervals, beta):
    """(precision, recall, f-measure, average overlap ratio) of the pairs ``m`` among the (non-empty) note lists."""
    p, r = len(m) / len(est_intervals), len(m) / len(ref_intervals)
    f = (1 + beta ** 2) * p * r / (beta ** 2 * p + r) if (p + r) > 0 else 0.0
    ratios = []
    for i, j in m:
        (rs, re_), (es, ee) = ref_intervals[i], est_intervals[j]
        ratios.append((min(re_, ee) - max(rs, es)) / (max(re_, ee) - min(rs, es)))
    return p, r, f, float(np.mean(ratios)) if ratios else 0.0


# ---------------------------------------------------------------------------------------------
# the same metrics without the host's per-frame lists and dense note matrices
# ---------------------------------------------------------------------------------------------
def match_notes_sparse(ref_intervals, ref_pitches, est_intervals, est_pitches, onset_tolerance=0.05, pitch_tolerance=50.0,
                       offset_ratio=0.2, offset_min_tolerance=0.05):
    """``match_notes`` without an N_ref x N_est matrix: same arguments, same pair list.

    Only pairs whose onsets lie within the tolerance can hit, so the candidates of a reference note are the estimates in a window
    of the onset-sorted list (the window is a millisecond wider than the tolerance: the dense route rounds the distance to 0.1 ms
    before it compares).  On the frame grid that is the estimates at most one hop (0.032 s <= 0.05 s < 0.064 s) away.  The float64
    onset, pitch and offset tests of ``match_notes`` are then applied to the candidates with the same expressions, and the hits go
    into a CSR matrix with the ``indptr`` / ``indices`` that ``csr_matrix(hit)`` has (rows in order, columns ascending), so
    ``maximum_bipartite_matching`` walks the same graph and returns the same matching, not just one of the same size."""
    ref_intervals = np.asarray(ref_intervals, dtype=np.float64).reshape(-1, 2)
    est_intervals = np.asarray(est_intervals, dtype=np.float64).reshape(-1, 2)
    n_ref, n_est = len(ref_intervals), len(est_intervals)
    if n_ref == 0 or n_est == 0:
        return []
    ref_pitches, est_pitches = np.asarray(ref_pitches), np.asarray(est_pitches)
    order = np.argsort(est_intervals[:, 0], kind='stable')
    sorted_on = est_intervals[order, 0]
    window = onset_tolerance + 1e-3
    lo = np.searchsorted(sorted_on, ref_intervals[:, 0] - window, side='left')
    hi = np.searchsorted(sorted_on, ref_intervals[:, 0] + window, side='right')
    per_ref = hi - lo
    rows = np.repeat(np.arange(n_ref), per_ref)
    first = np.cumsum(per_ref) - per_ref
    cols = order[np.repeat(lo, per_ref) + (np.arange(per_ref.sum()) - np.repeat(first, per_ref))]
    hit = np.around(np.abs(ref_intervals[rows, 0] - est_intervals[cols, 0]), N_DECIMALS) <= onset_tolerance
    rows, cols = rows[hit], cols[hit]
    hit = np.abs(1200.0 * (np.log2(ref_pitches)[rows] - np.log2(est_pitches)[cols])) <= pitch_tolerance
    rows, cols = rows[hit], cols[hit]
    if offset_ratio is not None:
        offset_d = np.around(np.abs(ref_intervals[rows, 1] - est_intervals[cols, 1]), N_DECIMALS)
        tol = offset_ratio * (ref_intervals[:, 1] - ref_intervals[:, 0])
        tol[tol <= offset_min_tolerance] = offset_min_tolerance
        hit = offset_d <= tol[rows]
        rows, cols = rows[hit], cols[hit]
    by_row_col = np.lexsort((cols, rows))
    rows, cols = rows[by_row_col], cols[by_row_col]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_ref))]).astype(np.int32)
    graph = csr_matrix((np.ones(len(cols), dtype=bool), cols.astype(np.int32), indptr), shape=(n_ref, n_est))
    match = maximum_bipartite_matching(graph, perm_type='column')
    return [(i, int(j)) for i, j in enumerate(match) if j >= 0]


def _frame_metrics_from_counts(counts):
    """The 14-key dict of ``evaluate_frames`` from its fourteen integer sums (plain seven, chroma seven): same float64 expressions,
    same zero guards."""
    out = {}
    for pre, (tp, n_ref, n_est, sub, miss, fa, tot) in (('', counts[:7]), ('Chroma ', counts[7:])):
        out[pre + 'Precision'] = tp / n_est if n_est else 0.0
        out[pre + 'Recall'] = tp / n_ref if n_ref else 0.0
        out[pre + 'Accuracy'] = tp / (n_est + n_ref - tp) if (n_est + n_ref - tp) else 0.0
        out[pre + 'Substitution Error'] = sub / n_ref if n_ref else 0.0
        out[pre + 'Miss Error'] = miss / n_ref if n_ref else 0.0
        out[pre + 'False Alarm Error'] = fa / n_ref if n_ref else 0.0
        out[pre + 'Total Error'] = tot / n_ref if n_ref else 0.0
    return out


def frame_counts_device(ref_roll, est_roll):
    """The fourteen integer sums behind ``evaluate_frames_device`` (rv_eval_frame_counts: plain tp, n_ref, n_est, substitutions, misses,
    false alarms, total, then the chroma seven) of two uint8 [T, 88] rolls on the device, as a list of Python ints."""
    _lib.need_gpu(ref_roll, est_roll)
    if ref_roll.dtype != torch.uint8 or est_roll.dtype != torch.uint8:
        raise TypeError('evaluate_frames_device: uint8 rolls expected')
    if ref_roll.dim() != 2 or ref_roll.shape[1] != 88 or ref_roll.shape != est_roll.shape or ref_roll.device != est_roll.device:
        raise ValueError('evaluate_frames_device: reference and estimate must be [T, 88] rolls of one song on one device')
    ref, est = ref_roll.contiguous(), est_roll.contiguous()
    ref = ref.clone() if ref.data_ptr() % 8 else ref
    est = est.clone() if est.data_ptr() % 8 else est
    T, dev = ref.shape[0], ref.device
    with torch.cuda.device(dev):
        ws_bytes = _lib.load().rv_eval_workspace_bytes(T)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        out = torch.empty(14, dtype=torch.int64, device=dev)
        _lib.call('rv_eval_frame_counts', ref.data_ptr(), est.data_ptr(), T, out.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream())
        return out.tolist()


def evaluate_frames_device(ref_roll, est_roll):
    """``evaluate_frames`` of two uint8 [T, 88] rolls on the device (the painted rolls of ``extract_notes_wo_velocity_device``):
    rv_eval_frame_counts sums the integer counters, the ratios are formed here in float64.  On the 88 piano keys a frame's match
    count is the popcount of ref & est, and the chroma count the sum over the 12 pitch classes of min(ref_k, est_k) -- the values
    the host's greedy matching within half a semitone arrives at -- so the result equals ``evaluate_frames`` value for value."""
    return _frame_metrics_from_counts(frame_counts_device(ref_roll, est_roll))


def average_precision_device(y_true, score):
    """scikit-learn's ``average_precision_score`` (binary labels, positive = 1) with the sort and the cumulative sums on the
    tensors' device: AP = sum_n (R_n - R_{n-1}) P_n over the DISTINCT score values in descending order, P_n and R_n the precision
    and recall of "score >= that value".  The counts are exact integers; the ratios and their sum are float64."""
    y = (y_true.reshape(-1) == 1)
    s = score.reshape(-1).to(y.device)
    if s.numel() != y.numel() or s.numel() == 0:
        raise ValueError('average_precision_device: labels and scores must have the same non-zero number of elements')
    s, idx = torch.sort(s, descending=True)
    tps = torch.cumsum(y[idx].to(torch.int64), 0)
    last = torch.ones_like(s, dtype=torch.bool)                         # last position of each run of equal scores
    last[:-1] = s[1:] != s[:-1]
    tps = tps[last].to(torch.float64)
    seen = (torch.nonzero(last).reshape(-1) + 1).to(torch.float64)      # tps + fps
    if float(tps[-1]) == 0.0:                                           # no positive label: sklearn's recall-is-one convention gives 0
        return 0.0
    precision = tps / seen
    recall = tps / tps[-1]
    step = recall - torch.cat([recall.new_zeros(1), recall[:-1]])
    return float((step * precision).sum())


# ---------------------------------------------------------------------------------------------
# the reference's evaluation loop
# ---------------------------------------------------------------------------------------------
def _to_eval_units(pitches, intervals):
    scaling = HOP_LENGTH / SAMPLE_RATE
    i = (np.asarray(intervals) * scaling).reshape(-1, 2)
    p = np.array([midi_to_hz(MIN_MIDI + midi) for midi in pitches])
    return p, i


def _frames_to_eval_units(t, freqs):
    scaling = HOP_LENGTH / SAMPLE_RATE
    return t.astype(np.float64) * scaling, [np.array([midi_to_hz(MIN_MIDI + midi) for midi in f]) for f in freqs]


Song = namedtuple('Song', 'label losses pred spec lab_on lab_fr ref_on est_on')


def _songs(data, model, onset, pseudo_onset, VAT, device_metrics):
    """The per-song pass that evaluation and tuning share: exactly one eval-mode ``run_on_batch`` per song of ``data``.  Yields a ``Song``:
    the label, the losses, ``pred`` with its rolls relu'd and squeezed to [T, 88], the spectrogram (``run_on_batch``'s third result), the
    label rolls -- moved to the prediction's device under ``device_metrics`` only -- and the onset rolls the reference and the estimate
    are decoded from: the label's and the predicted onsets (``pseudo_onset``: the label's for both), or with ``onset=False`` the two
    frame rolls.  Whatever else a metric needs of a song belongs here."""
    for label in data:
        pred, losses, spec = model.run_on_batch(label, None, False) if VAT else model.run_on_batch(label)
        for key in ('frame', 'onset', 'frame2', 'onset2'):
            if pred.get(key) is not None:
                pred[key] = pred[key].detach().squeeze(0).relu()
        lab_on, lab_fr = label['onset'].squeeze(0), label['frame'].squeeze(0)
        if device_metrics:
            lab_on, lab_fr = lab_on.to(pred['frame'].device), lab_fr.to(pred['frame'].device)
        if onset:
            yield Song(label, losses, pred, spec, lab_on, lab_fr, lab_on, lab_on if pseudo_onset else pred['onset'])
        else:
            yield Song(label, losses, pred, spec, lab_on, lab_fr, lab_fr, pred['frame'])


def _eval_units(notes, shape, device_metrics):
    """A decode (pitches, intervals, velocities, painted) of ``NoteDecoder`` in the units of the metrics: (pitches in Hz, intervals in
    seconds, frames) -- ``frames`` the painted roll under ``device_metrics``, else the (times, pitch lists) of ``notes_to_frames``."""
    pitches, intervals, _, painted = notes
    frames = painted if device_metrics else _frames_to_eval_units(*notes_to_frames(pitches, intervals, shape))
    return _to_eval_units(pitches, intervals) + (frames,)


def _song_metrics(ref, est, device_metrics):
    """The metrics of one estimate of one song, ``ref`` and ``est`` as ``_eval_units`` makes them: ((P, R, F, overlap) of the notes, the
    same with offsets, the dictionary of ``evaluate_frames``, the frame F1).  ``device_metrics`` picks ``match_notes_sparse`` and
    ``evaluate_frames_device`` over ``match_notes`` and ``evaluate_frames``: same values."""
    (p_ref, i_ref, f_ref), (p_est, i_est, f_est) = ref, est
    matcher = match_notes_sparse if device_metrics else match_notes
    note = evaluate_notes(i_ref, p_ref, i_est, p_est, offset_ratio=None, match=matcher)
    with_offsets = evaluate_notes(i_ref, p_ref, i_est, p_est, match=matcher)
    fm = evaluate_frames_device(f_ref, f_est) if device_metrics else evaluate_frames(*f_ref, *f_est)
    return note, with_offsets, fm, hmean([fm['Precision'] + eps, fm['Recall'] + eps]) - eps


def _decoders(onset_threshold, frame_threshold, rule, min_frames, bridge_gap, hmm, onset):
    """The decoders of (the labels, the estimate, the estimate of the ``_2`` pass); a bad argument raises here, before any song is touched.
    The labels are decoded at 0.5 / 0.5 and ``rule`` without clean-up or model; the ``_2`` pass at the decoder's default rule, whatever
    ``rule`` says, as in the reference."""
    est = dict(min_frames=min_frames, bridge_gap=bridge_gap, hmm=hmm, onset=onset)
    return (NoteDecoder(rule=rule), NoteDecoder(onset_threshold, frame_threshold, rule, **est),
            NoteDecoder(onset_threshold, frame_threshold, **est))


def _evaluate_song(metrics, song, decoders, reconstruction, device_metrics, save_path, velocities=(None, None)):
    """``evaluate_wo_velocity`` for one ``Song``: appends its values to ``metrics`` and returns the decodes (reference, estimate) in frame
    units.  ``velocities``: the velocity rolls the two decodes read per note, if any."""
    from sklearn.metrics import average_precision_score
    label, losses, pred, _, lab_on, lab_fr, ref_on, est_on = song
    decode_ref, decode_est, decode_est2 = decoders
    for key, loss in losses.items():
        metrics[key].append(loss.item())
    ref_notes = decode_ref(ref_on, lab_fr, velocities[0], device_metrics)
    est_notes = decode_est(est_on, pred['frame'], velocities[1], device_metrics)
    ref = _eval_units(ref_notes, lab_fr.shape, device_metrics)
    est = _eval_units(est_notes, pred['frame'].shape, device_metrics)

    def average_precision(score):
        if device_metrics:
            return average_precision_device(lab_fr.flatten(), score.flatten())
        return average_precision_score(lab_fr.cpu().flatten().numpy(), score.cpu().flatten().numpy())

    def block(suffix, est):
        note, with_offsets, fm, f1 = _song_metrics(ref, est, device_metrics)
        for tag, values in (('note', note), ('note-with-offsets', with_offsets)):
            for k, v in zip(('precision', 'recall', 'f1', 'overlap'), values):
                metrics[f'metric/{tag}/{k}{suffix}'].append(v)
        metrics['metric/frame/f1' + suffix].append(f1)
        return fm

    frame_metrics = block('', est)
    metrics['metric/MusicNet/micro_avg_P'].append(average_precision(pred['frame']))
    if reconstruction and pred.get('frame2') is not None:
        fm2 = block('_2', _eval_units(decode_est2(pred['onset2'], pred['frame2'], None, device_metrics), pred['frame2'].shape, device_metrics))
        frame_metrics['Precision_2'], frame_metrics['Recall_2'], frame_metrics['accuracy_2'] = \
            fm2['Precision'], fm2['Recall'], fm2['Accuracy']
        metrics['metric/MusicNet/micro_avg_P2'].append(average_precision(pred['frame2']))
    for key, value in frame_metrics.items():
        metrics['metric/frame/' + key.lower().replace(' ', '_')].append(value)
    if save_path is not None:
        os.makedirs(save_path, exist_ok=True)
        path = label['path'][0] if isinstance(label['path'], (list, tuple)) else label['path']
        stem = os.path.join(save_path, os.path.basename(str(path)))
        save_pianoroll(stem + '.label.png', lab_on, lab_fr)
        save_pianoroll(stem + '.pred.png', pred['onset'] if pred.get('onset') is not None else pred['frame'], pred['frame'])
        save_midi(stem + '.pred.mid', est[0], est[1], [127] * len(est[0]))
    return ref_notes, est_notes


def evaluate_wo_velocity(data, model, onset_threshold=0.5, frame_threshold=0.5, save_path=None, reconstruction=True,
                         onset=True, pseudo_onset=False, rule='rule2', VAT=False, device_metrics=False, min_frames=1, bridge_gap=0,
                         hmm=None):
    """model/evaluate_functions.py:20-127: whole-song evaluation; returns a dict of lists with the reference's keys
    (losses, metric/note/*, metric/note-with-offsets/*, metric/frame/*, metric/MusicNet/micro_avg_P, and the *_2
    variants of the reconstruction pass).  ``save_path``: per song `<basename>.pred.mid` (the transcription, reconvat_amd/midi.py)
    and the `<basename>.label.png` / `.pred.png` piano rolls (model/utils.py:61-80), as the reference writes them (:119-126).

    ``device_metrics=True`` computes the same dictionary where the posteriorgrams are: notes and painted rolls by the
    device side of ``NoteDecoder``, frame metrics by ``evaluate_frames_device``, note matching by ``match_notes_sparse``, AP by
    ``average_precision_device``; the per-frame lists of ``notes_to_frames`` are never built.  The model must be on a HIP device.

    ``min_frames`` / ``bridge_gap``: the note clean-up of ``extract_notes_wo_velocity``, applied to the decodes of the
    estimate -- the ``_2`` pass included -- on either path; the labels are decoded without it.

    ``hmm``: a ``hmm.NoteHMM``.  Every decode of the estimate, the ``_2`` pass included, is then the Viterbi decode of that
    model followed by the same clean-up; the labels are decoded as without it, and the two threshold arguments are unused (the model
    carries its own).  A model that uses onsets cannot decode ``onset=False``: ValueError before any song is touched."""
    decoders = _decoders(onset_threshold, frame_threshold, rule, min_frames, bridge_gap, hmm, onset)
    metrics = defaultdict(list)
    for song in _songs(data, model, onset, pseudo_onset, VAT, device_metrics):
        _evaluate_song(metrics, song, decoders, reconstruction, device_metrics, save_path)
    return metrics


# ---------------------------------------------------------------------------------------------
# note metrics with velocity (mir_eval.transcription_velocity.precision_recall_f1_overlap)
# ---------------------------------------------------------------------------------------------
def evaluate_notes_with_velocity(ref_intervals, ref_pitches, ref_velocities, est_intervals, est_pitches, est_velocities,
                                 onset_tolerance=0.05, pitch_tolerance=50.0, offset_ratio=0.2, offset_min_tolerance=0.05,
                                 velocity_tolerance=0.1, beta=1.0):
    """(precision, recall, f-measure, average overlap ratio) over the matched pairs whose velocities agree.  The pairs come from
    ``match_notes_sparse``; the reference velocities are mapped to (v - min) / max(1, max - min); slope and intercept of the least
    squares line from the matched estimated velocities to the matched (mapped) reference velocities are fitted, and a pair survives
    if |slope est + intercept - ref| < velocity_tolerance.  An empty matching, or no notes on either side, gives zeros."""
    ref_intervals = np.asarray(ref_intervals, dtype=np.float64).reshape(-1, 2)
    est_intervals = np.asarray(est_intervals, dtype=np.float64).reshape(-1, 2)
    ref_v = np.asarray(ref_velocities, dtype=np.float64).reshape(-1)
    est_v = np.asarray(est_velocities, dtype=np.float64).reshape(-1)
    if len(ref_v) != len(ref_intervals) or len(est_v) != len(est_intervals):
        raise ValueError('evaluate_notes_with_velocity: one velocity per note expected')
    if len(ref_pitches) == 0 or len(est_pitches) == 0:
        return 0.0, 0.0, 0.0, 0.0
    m = match_notes_sparse(ref_intervals, ref_pitches, est_intervals, est_pitches, onset_tolerance, pitch_tolerance, offset_ratio,
                           offset_min_tolerance)
    if not m:
        return 0.0, 0.0, 0.0, 0.0
    ref_v = (ref_v - ref_v.min()) / max(1.0, ref_v.max() - ref_v.min())
    ri, ej = np.array([i for i, _ in m]), np.array([j for _, j in m])
    design = np.stack([est_v[ej], np.ones(len(m))], axis=1)
    slope, intercept = np.linalg.lstsq(design, ref_v[ri], rcond=None)[0]
    keep = np.abs(slope * est_v[ej] + intercept - ref_v[ri]) < velocity_tolerance
    return _scores_of_matching([pair for pair, k in zip(m, keep) if k], ref_intervals, est_intervals, beta)


def evaluate_with_velocity(data, model, head, onset_threshold=0.5, frame_threshold=0.5, rule='rule2', min_frames=1, bridge_gap=0,
                           velocity_tolerance=0.1, save_path=None, reconstruction=True, onset=True, pseudo_onset=False, VAT=False, hmm=None):
    """``evaluate_wo_velocity``'s dictionary (its arguments, always ``device_metrics=True``) plus ``metric/note-with-velocity/*`` and
    ``metric/note-with-offsets-and-velocity/*`` (precision, recall, f1, overlap per song), in one pass: one ``run_on_batch`` per song, and
    both halves of the dictionary describe the same note lists -- with ``hmm`` those of its Viterbi path, whose velocities are means over
    the path's ONSET frames.  The estimate's velocity roll is ``head`` (velocity.VelocityHead) on the spectrogram of the same audio, read
    per note by the decoder; the reference's is ``label['velocity']`` read the same way.  After per-clip normalisation only the
    rescaled comparison made by ``evaluate_notes_with_velocity`` is meaningful.  The model and the head must be on a HIP device; a head of
    another front end is refused before any song is touched."""
    head.check_front_end(model)
    decoders = _decoders(onset_threshold, frame_threshold, rule, min_frames, bridge_gap, hmm, onset)
    metrics = defaultdict(list)
    for song in _songs(data, model, onset, pseudo_onset, VAT, True):
        spec = song.spec
        if spec.shape[-1] != head.centres.numel():
            raise ValueError(f'evaluate_with_velocity: the model returned a spectrogram of shape {tuple(spec.shape)}; the head expects '
                             f'{head.centres.numel()} bins on the last axis')
        with torch.no_grad():
            roll = head(spec.reshape(1, -1, spec.shape[-1])).squeeze(0)
        lab_vel = song.label['velocity'].squeeze(0).to(roll.device)
        ref, est = _evaluate_song(metrics, song, decoders, reconstruction, True, save_path, (lab_vel, roll))
        (p_ref, i_ref), (p_est, i_est) = _to_eval_units(*ref[:2]), _to_eval_units(*est[:2])
        for tag, ratio in (('note-with-velocity', None), ('note-with-offsets-and-velocity', 0.2)):
            res = evaluate_notes_with_velocity(i_ref, p_ref, 128.0 * ref[2], i_est, p_est, est[2], offset_ratio=ratio,     # MIDI units: the map divides by the range
                                               velocity_tolerance=velocity_tolerance)
            for k, v in zip(('precision', 'recall', 'f1', 'overlap'), res):
                metrics[f'metric/{tag}/{k}'].append(v)
    return metrics


# ---------------------------------------------------------------------------------------------
# onset timing against exact note lists
# ---------------------------------------------------------------------------------------------
TIMING_TOLERANCES = ((0.05, '50ms'), (0.01, '10ms'))


def evaluate_timing(data, model, decoder=None, refine=False, lead=0, device_metrics=False):
    """How close the transcribed onsets are to the EXACT onsets of a corpus that carries its note lists (``RenderedScores.scores``: tsv
    rows in seconds) -- ``evaluate_wo_velocity`` decodes its reference from the label roll and cannot see anything finer than a frame.
    One eval-mode ``run_on_batch`` per whole track (``_songs``), the notes of ``decoder`` (a ``NoteDecoder``, default rule2 at 0.5 / 0.5)
    and, with ``refine``, their onsets moved by ``onset_time.refine_intervals(..., lead)`` on the track's audio where it is (the kernel on
    a HIP device).  Per song: ``metric/timing/{precision,recall,f1}@50ms`` and ``@10ms`` (``evaluate_notes`` against the exact rows,
    onsets only) and ``metric/timing/onset_error_{mean,median}_ms`` over the pairs matched at 50 ms (0 without a pair).
    ``device_metrics`` picks the device decoder and ``match_notes_sparse``: same values.  ValueError for a dataset without ``scores`` or
    one that crops its tracks."""
    from . import onset_time
    scores = getattr(data, 'scores', None)
    if scores is None or len(scores) != len(data):
        raise ValueError('evaluate_timing needs a dataset with exact note lists: RenderedScores and its `scores`')
    if getattr(data, 'sequence_length', None) is not None:
        raise ValueError('evaluate_timing works on whole tracks (sequence_length=None): the note lists count from the first sample')
    decoder = NoteDecoder(rule='rule2') if decoder is None else decoder
    lead = onset_time._lead(lead)
    matcher = match_notes_sparse if device_metrics else match_notes
    metrics = defaultdict(list)
    for rows, song in zip(scores, _songs(data, model, True, False, False, device_metrics)):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
        p_ref, i_ref = midi_to_hz(rows[:, 2]), rows[:, :2]
        pitches, intervals, _, _ = decoder(song.est_on, song.pred['frame'], None, device_metrics)
        if refine:
            audio = song.label['audio'].reshape(-1)
            i_est = onset_time.refine_intervals(audio, pitches, intervals, lead, device=audio.is_cuda)
            p_est = _to_eval_units(pitches, intervals)[0]
        else:
            p_est, i_est = _to_eval_units(pitches, intervals)
        for tol, tag in TIMING_TOLERANCES:
            p, r, f, _ = evaluate_notes(i_ref, p_ref, i_est, p_est, onset_tolerance=tol, offset_ratio=None, match=matcher)
            for k, v in zip(('precision', 'recall', 'f1'), (p, r, f)):
                metrics[f'metric/timing/{k}@{tag}'].append(v)
        pairs = matcher(i_ref, p_ref, i_est, p_est, 0.05, 50.0, None, 0.05) if len(p_ref) and len(p_est) else []
        err = np.array([abs(i_est[j, 0] - i_ref[i, 0]) for i, j in pairs]) * 1e3
        metrics['metric/timing/onset_error_mean_ms'].append(float(err.mean()) if len(err) else 0.0)
        metrics['metric/timing/onset_error_median_ms'].append(float(np.median(err)) if len(err) else 0.0)
    return metrics


# ---------------------------------------------------------------------------------------------
# decoding thresholds chosen on a validation set
# ---------------------------------------------------------------------------------------------
SWEEP_KEYS = ('n_est', 'matched', 'matched_with_offsets', 'frame_tp', 'frame_est')      # int64 [n_on, n_fr] each; order of rv_eval_sweep
SWEEP_CRITERIA = ('note_f1', 'note_with_offsets_f1', 'frame_f1')
MAX_SWEEP_THRESHOLDS = 32
_SCALING = HOP_LENGTH / SAMPLE_RATE
# the sweep kernel pairs a reference note with estimates that start at most one frame away: that IS the 50 ms onset tolerance of
# match_notes on this frame grid (its rounded distances are 0.032 and 0.064)
assert np.around(_SCALING, N_DECIMALS) <= 0.05 < np.around(2 * _SCALING, N_DECIMALS)


def _sweep_grid(onset_thresholds, frame_thresholds):
    on = np.atleast_1d(np.asarray(onset_thresholds, dtype=np.float32))
    fr = np.atleast_1d(np.asarray(frame_thresholds, dtype=np.float32))
    if on.ndim != 1 or fr.ndim != 1 or not 1 <= len(on) <= MAX_SWEEP_THRESHOLDS or not 1 <= len(fr) <= MAX_SWEEP_THRESHOLDS:
        raise ValueError(f'threshold lists must hold 1..{MAX_SWEEP_THRESHOLDS} values each, got {on.shape} and {fr.shape}')
    return on, fr


def sweep_counts_host(onset_ref, frame_ref, onset_pred, frame_pred, onset_thresholds, frame_thresholds, rule='rule2', min_frames=1,
                      bridge_gap=0):
    """The integer counters behind the note and frame metrics of one song at every pair of a threshold grid, by a plain loop over the
    host functions: the labels are decoded once at 0.5 / 0.5, the posteriorgrams at every pair (``extract_notes_wo_velocity``,
    float32 ``x > threshold``); ``match_notes`` without and with the offset test gives the two match counts, ``notes_to_frames`` the
    painted frames.  Returns int64 [n_on, n_fr] arrays ``n_est``, ``matched``, ``matched_with_offsets``, ``frame_tp`` (frames painted by
    reference and estimate), ``frame_est``, and the ints ``n_ref`` and ``frame_ref``.  ``min_frames`` / ``bridge_gap`` clean
    up the notes of the estimate, never those of the labels.  The yardstick of ``sweep_counts_device``."""
    on_thr, fr_thr = _sweep_grid(onset_thresholds, frame_thresholds)
    shape = tuple(frame_ref.shape)
    p_ref, i_ref = extract_notes_wo_velocity(onset_ref, frame_ref, rule=rule)
    _, f_ref = notes_to_frames(p_ref, i_ref, shape)
    pr, ir = _to_eval_units(p_ref, i_ref)
    out = {k: np.zeros((len(on_thr), len(fr_thr)), np.int64) for k in SWEEP_KEYS}
    for a, t_on in enumerate(on_thr):
        for b, t_fr in enumerate(fr_thr):
            p_est, i_est = extract_notes_wo_velocity(onset_pred, frame_pred, float(t_on), float(t_fr), rule=rule, min_frames=min_frames,
                                                     bridge_gap=bridge_gap)
            _, f_est = notes_to_frames(p_est, i_est, shape)
            pe, ie = _to_eval_units(p_est, i_est)
            out['n_est'][a, b] = len(pe)
            out['matched'][a, b] = len(match_notes(ir, pr, ie, pe, offset_ratio=None))
            out['matched_with_offsets'][a, b] = len(match_notes(ir, pr, ie, pe))
            out['frame_tp'][a, b] = sum(len(np.intersect1d(r, e)) for r, e in zip(f_ref, f_est))
            out['frame_est'][a, b] = sum(len(e) for e in f_est)
    out['n_ref'], out['frame_ref'] = len(pr), sum(len(r) for r in f_ref)
    return out


def _offset_slack(intervals):
    """Per reference note (frame units [N, 2]) how many frames an estimate may end before / after the note's end and still pass
    ``match_notes``' offset test -- that test evaluated here, once, with its own float64 expressions on times ``frame * 0.032``, so
    the device compares integers.  The rounded distance grows with the frame difference, so the admissible differences are an
    interval around 0; its two edges are looked for next to tolerance / hop."""
    ref = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
    times = (ref * _SCALING).reshape(-1, 2)
    tol = 0.2 * (times[:, 1] - times[:, 0])
    tol[tol <= 0.05] = 0.05
    guess = np.floor(tol / _SCALING).astype(np.int64)
    slack = []
    for sign in (-1, 1):
        best = np.zeros(len(ref), np.int64)
        for step in range(-2, 3):
            k = np.maximum(guess + step, 0)
            ok = np.around(np.abs(times[:, 1] - (ref[:, 1] + sign * k) * _SCALING), N_DECIMALS) <= tol
            best = np.where(ok, np.maximum(best, k), best)
        slack.append(best)
    return np.stack(slack, axis=1)


def sweep_counts_device(onset_ref, frame_ref, onset_pred, frame_pred, onset_thresholds, frame_thresholds, rule='rule2', min_frames=1,
                        bridge_gap=0):
    """``sweep_counts_host`` where the posteriorgrams are (csrc/eval.hip): same arguments, same result, two
    launches for the whole grid and one (min_frames, bridge_gap).  The labels are decoded once by ``rv_eval_decode_clean`` at (1, 0);
    their notes go back to the device sorted by pitch with the offset tolerance of each as a number of frames (``_offset_slack``), and
    ``rv_eval_sweep_clean`` thresholds the rolls into bit masks once per threshold and counts kept notes, matches and painted frames
    per pair.  Raises on a CPU tensor: no fallback."""
    if rule not in _RULES:
        raise NameError('Please enter the correct rule name')
    min_frames, bridge_gap = _cleanup_args(min_frames, bridge_gap)
    on_thr, fr_thr = _sweep_grid(onset_thresholds, frame_thresholds)
    onset_ref, frame_ref, on, fr = _device_rolls(onset_ref, frame_ref, onset_pred, frame_pred)
    p_ref, i_ref, roll_ref = extract_notes_wo_velocity_device(onset_ref, frame_ref, rule=rule)
    T, dev, n_ref = on.shape[0], on.device, len(p_ref)
    rows = np.zeros((max(n_ref, 1), 5), np.int32)
    if n_ref:
        order = np.lexsort((i_ref[:, 0], p_ref))
        rows[:, 0], rows[:, 1], rows[:, 2] = i_ref[order, 0], p_ref[order], i_ref[order, 1]
        rows[:, 3:] = np.minimum(_offset_slack(i_ref[order]), T)
    n_on, n_fr = len(on_thr), len(fr_thr)
    with torch.cuda.device(dev):
        ws_bytes = _lib.load().rv_eval_sweep_workspace_bytes(T, n_on, n_fr)
        if ws_bytes <= 0:
            raise ValueError(f'rv_eval_sweep_clean: no workspace for T = {T} and a {n_on} x {n_fr} grid')
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        thr = torch.from_numpy(np.concatenate([on_thr, fr_thr])).to(dev)
        ref_notes = torch.from_numpy(rows).to(dev)
        counts = torch.empty((n_on, n_fr, len(SWEEP_KEYS)), dtype=torch.int64, device=dev)
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.call('rv_eval_sweep_clean', on.data_ptr(), fr.data_ptr(), T, thr.data_ptr(), n_on, thr.data_ptr() + 4 * n_on, n_fr,
                  _RULES[rule], min_frames, bridge_gap, ref_notes.data_ptr(), n_ref, roll_ref.data_ptr(), counts.data_ptr(),
                  totals.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream())
        counts, totals = counts.cpu().numpy(), totals.tolist()
    out = {k: np.ascontiguousarray(counts[:, :, c]) for c, k in enumerate(SWEEP_KEYS)}
    out['n_ref'], out['frame_ref'] = int(totals[0]), int(totals[1])
    return out


def sweep_metrics(counts, a, b):
    """The nine metrics of one song at grid point (a, b) from its sweep counters, with the float64 expressions and zero guards of
    ``evaluate_notes`` (beta = 1), ``evaluate_frames`` and the frame F1 of ``evaluate_wo_velocity``."""
    n_ref, n_est, beta = int(counts['n_ref']), int(counts['n_est'][a, b]), 1.0
    out = {}
    for name, key in (('note', 'matched'), ('note_with_offsets', 'matched_with_offsets')):
        m = int(counts[key][a, b])
        if n_ref == 0 or n_est == 0:
            p = r = f = 0.0
        else:
            p, r = m / n_est, m / n_ref
            f = (1 + beta ** 2) * p * r / (beta ** 2 * p + r) if (p + r) > 0 else 0.0
        out[name + '_precision'], out[name + '_recall'], out[name + '_f1'] = p, r, f
    tp, fe, fr = int(counts['frame_tp'][a, b]), int(counts['frame_est'][a, b]), int(counts['frame_ref'])
    out['frame_precision'] = tp / fe if fe else 0.0
    out['frame_recall'] = tp / fr if fr else 0.0
    out['frame_f1'] = hmean([out['frame_precision'] + eps, out['frame_recall'] + eps]) - eps
    return out


def best_threshold_index(values, onset_thresholds, frame_thresholds):
    """Index (a, b) of the largest value; ties go to the pair nearest (0.5, 0.5) in max-norm (rounded to 1e-6), then to the lowest a,
    then to the lowest b."""
    values = np.asarray(values, dtype=np.float64)
    far = np.round(np.maximum(np.abs(np.atleast_1d(np.asarray(onset_thresholds, np.float64)) - 0.5)[:, None],
                              np.abs(np.atleast_1d(np.asarray(frame_thresholds, np.float64)) - 0.5)[None, :]), 6)
    best = None
    for a in range(values.shape[0]):
        for b in range(values.shape[1]):
            key = (-values[a, b], far[a, b], a, b)
            if best is None or key < best:
                best = key
    return best[2], best[3]


MAX_CLEANUPS = 8


def tune_thresholds(data, model, onset_thresholds, frame_thresholds, criterion='note_f1', onset=True, pseudo_onset=False, rule='rule2',
                    device_metrics=True, VAT=False, cleanups=((1, 0),)):
    """Choose ``onset_threshold`` / ``frame_threshold`` on a validation set.  One eval-mode ``run_on_batch`` per song of ``data`` (as
    in ``evaluate_wo_velocity``; ``onset`` / ``pseudo_onset`` / ``rule`` / ``VAT`` mean what they mean there), then the sweep counters of
    the song over the whole grid -- ``sweep_counts_device`` (``device_metrics=True``, model on a HIP device) or ``sweep_counts_host``
    -- and from them per-song precision / recall / F1 of notes, notes with offsets and frames (``sweep_metrics``), averaged over the
    songs with ``np.mean`` like the lists of ``evaluate_wo_velocity``: every grid value equals the mean of the matching
    ``evaluate_wo_velocity`` list at that pair.

    ``cleanups``: 1..8 ``(min_frames, bridge_gap)`` pairs to choose among as well -- still one forward per song, then
    one sweep per pair.

    Returns ``{'onset_thresholds', 'frame_thresholds', 'grid': {metric: float64 [n_on, n_fr]}, 'criterion', 'best_index': (a, b),
    'onset_threshold', 'frame_threshold', 'best_value', 'songs', 'cleanups', 'grids', 'best_cleanup', 'min_frames', 'bridge_gap'}``.
    ``grids`` holds one grid dictionary per entry of ``cleanups``, ``best_cleanup`` is the index of the chosen entry and ``grid`` its
    grid.  The best triple maximises ``grids[c][criterion][a, b]`` (``note_f1``, ``note_with_offsets_f1`` or ``frame_f1``).  Ties go to
    the earliest entry of ``cleanups``, then to the pair nearest (0.5, 0.5) in max-norm (distances compared after rounding to 1e-6,
    so that 0.3 and 0.7 are equally far), then to the lowest onset index, then to the lowest frame index."""
    if criterion not in SWEEP_CRITERIA:
        raise ValueError(f'criterion must be one of {SWEEP_CRITERIA}, got {criterion!r}')
    on_thr, fr_thr = _sweep_grid(onset_thresholds, frame_thresholds)
    cleanups = [tuple(c) for c in cleanups]
    if not 1 <= len(cleanups) <= MAX_CLEANUPS or any(len(c) != 2 for c in cleanups):
        raise ValueError(f'cleanups must hold 1..{MAX_CLEANUPS} (min_frames, bridge_gap) pairs, got {cleanups}')
    cleanups = [_cleanup_args(*c) for c in cleanups]
    sweep = sweep_counts_device if device_metrics else sweep_counts_host
    per_song = [defaultdict(list) for _ in cleanups]
    for s in _songs(data, model, onset, pseudo_onset, VAT, device_metrics):
        rolls = (s.ref_on, s.lab_fr, s.est_on, s.pred['frame'])
        for (min_frames, bridge_gap), lists in zip(cleanups, per_song):
            counts = sweep(*rolls, on_thr, fr_thr, rule=rule, min_frames=min_frames, bridge_gap=bridge_gap)
            song = defaultdict(lambda: np.zeros((len(on_thr), len(fr_thr)), np.float64))
            for a in range(len(on_thr)):
                for b in range(len(fr_thr)):
                    for k, v in sweep_metrics(counts, a, b).items():
                        song[k][a, b] = v
            for k, v in song.items():
                lists[k].append(v)
    if not per_song[0]:
        raise ValueError('tune_thresholds: no song in the validation set')
    grids = []
    for lists in per_song:                                              # np.mean of the per-song list, cell by cell: the scripts' average
        grids.append({k: np.array([[np.mean([song[a, b] for song in v]) for b in range(len(fr_thr))] for a in range(len(on_thr))])
                      for k, v in lists.items()})
    best = [best_threshold_index(grid[criterion], onset_thresholds, frame_thresholds) for grid in grids]
    c = int(np.argmax([grid[criterion][ab] for grid, ab in zip(grids, best)]))      # argmax: the earliest of equal values
    a, b = best[c]
    return {'onset_thresholds': on_thr, 'frame_thresholds': fr_thr, 'grid': grids[c], 'criterion': criterion, 'best_index': (a, b),
            'onset_threshold': float(on_thr[a]), 'frame_threshold': float(fr_thr[b]), 'best_value': float(grids[c][criterion][a, b]),
            'songs': len(per_song[0][criterion]), 'cleanups': cleanups, 'grids': grids, 'best_cleanup': c,
            'min_frames': cleanups[c][0], 'bridge_gap': cleanups[c][1]}


MAX_HMM_SETS = 256
HMM_METRICS = ('note_precision', 'note_recall', 'note_f1', 'note_with_offsets_precision', 'note_with_offsets_recall',
               'note_with_offsets_f1', 'frame_precision', 'frame_recall', 'frame_f1')


def tune_hmm(data, model, hmms, criterion='note_f1', onset=True, pseudo_onset=False, device_metrics=True, VAT=False, min_frames=1,
             bridge_gap=0):
    """Choose a ``hmm.NoteHMM`` among ``hmms`` (1..256 of them; ``hmm.hmm_grid`` builds a product) on a validation set.
    One eval-mode ``run_on_batch`` per song of ``data``, as in ``tune_thresholds``; then, with ``device_metrics`` (model on a HIP device),
    one batched Viterbi decode per 16 sets (``viterbi_states_device``), else ``viterbi_states`` set by set, and ``hmm.path_notes`` of every
    path; the metric code of ``evaluate_wo_velocity`` runs per set, and the per-song values are averaged with ``np.mean``: every value equals the mean of the
    matching ``evaluate_wo_velocity(..., hmm=h)`` list.  The labels are decoded once per song, at rule2.

    Returns ``{'hmms', 'values': {metric: float64 [n]}, 'criterion', 'best_index', 'best', 'best_value', 'songs'}`` with the metrics of
    ``HMM_METRICS``; ``best`` maximises ``values[criterion]`` (``note_f1``, ``note_with_offsets_f1`` or ``frame_f1``), ties go to the lowest
    index."""
    if criterion not in SWEEP_CRITERIA:
        raise ValueError(f'criterion must be one of {SWEEP_CRITERIA}, got {criterion!r}')
    hmms = list(hmms)
    if not 1 <= len(hmms) <= MAX_HMM_SETS:
        raise ValueError(f'tune_hmm takes 1..{MAX_HMM_SETS} parameter sets, got {len(hmms)}')
    for h in hmms:
        if not isinstance(h, NoteHMM):
            raise TypeError(f'hmms must hold NoteHMM objects, got {type(h).__name__}')
        if not onset and h.use_onsets:
            raise ValueError('onset=False decodes the frame roll alone: every NoteHMM must have use_onsets=False')
    min_frames, bridge_gap = _cleanup_args(min_frames, bridge_gap)
    decode_ref = NoteDecoder(rule='rule2')
    per_song = defaultdict(list)                                        # metric -> one float64 [n] per song
    for s in _songs(data, model, onset, pseudo_onset, VAT, device_metrics):
        frame = s.pred['frame']
        ref = _eval_units(decode_ref(s.ref_on, s.lab_fr, None, device_metrics), s.lab_fr.shape, device_metrics)
        if device_metrics:                                              # all sets of the song in one batched call per 16
            paths = viterbi_states_device(s.est_on, frame, hmms)[0]
        else:
            paths = [viterbi_states(s.est_on, frame, *h.tables())[0] for h in hmms]
        decoded = [path_notes(states, None, min_frames, bridge_gap, device_metrics) for states in paths]
        song = {k: np.zeros(len(hmms), np.float64) for k in HMM_METRICS}
        for n, notes in enumerate(decoded):
            note, with_offsets, fm, f1 = _song_metrics(ref, _eval_units(notes, frame.shape, device_metrics), device_metrics)
            for name, (p, r, f, _) in (('note', note), ('note_with_offsets', with_offsets)):
                song[name + '_precision'][n], song[name + '_recall'][n], song[name + '_f1'][n] = p, r, f
            song['frame_precision'][n], song['frame_recall'][n], song['frame_f1'][n] = fm['Precision'], fm['Recall'], f1
        for k, v in song.items():
            per_song[k].append(v)
    if not per_song:
        raise ValueError('tune_hmm: no song in the validation set')
    values = {k: np.array([np.mean([s[n] for s in v]) for n in range(len(hmms))]) for k, v in per_song.items()}
    best = int(np.argmax(values[criterion]))                            # argmax: the lowest index of equal values
    return {'hmms': hmms, 'values': values, 'criterion': criterion, 'best_index': best, 'best': hmms[best],
            'best_value': float(values[criterion][best]), 'songs': len(per_song[criterion])}


def save_pianoroll(path, onsets, frames, onset_threshold=0.5, frame_threshold=0.5, zoom=4):
    """model/utils.py:61-80: RGB piano-roll diagram (onsets / frames / both, pitch upwards, `zoom` x stretched).  Needs PIL; without
    it the diagram is skipped (the MIDI file and the metrics do not depend on it)."""
    try:
        from PIL import Image
    except ImportError:
        return False
    on = (1 - (onsets.t() > onset_threshold).to(torch.uint8)).cpu()
    fr = (1 - (frames.t() > frame_threshold).to(torch.uint8)).cpu()
    both = 1 - (1 - on) * (1 - fr)
    image = torch.stack([on, fr, both], dim=2).flip(0).mul(255).numpy()
    image = Image.fromarray(image, 'RGB')
    image.resize((image.size[0], image.size[1] * zoom)).save(path)
    return True
