"""decoding.NoteDecoder against the public functions it stands behind, and the per-song pass of evaluate.py (no GPU): the decoder's
result must equal ``extract_notes_wo_velocity`` / ``extract_notes_with_velocity`` / ``hmm.extract_notes_hmm`` for the same arguments;
evaluation and both tuners run the model exactly once per song; and the rules at which the ``_2`` pass and ``tune_hmm`` decode stay
what they were.  tests/test_note_decoder_gpu.py runs the same matrix with ``device=True``."""
import itertools

import numpy as np
import pytest
import torch

import sweep_cases as sc
from reconvat_amd import NoteHMM, decoding as md, evaluate as ev, hmm as nh

T = 130                                         # two whole 64-frame tiles (or HMM chunks) and a remainder
SEEDS = (3, 4)
RULES = ('rule1', 'rule2')
CLEANUPS = ((1, 0), (2, 1))
HMMS = (None, NoteHMM(), NoteHMM(0.3, 0.7, 0.0, 1.0, 2.0))
MATRIX = list(itertools.product(SEEDS, HMMS, RULES, CLEANUPS, (False, True)))


def rolls(T, seed):
    """(onset, frame, velocity) float32 [T, 88] tensors: the predictions of sweep_cases.random_rolls and a uniform velocity roll."""
    _, _, on_p, fr_p = sc.random_rolls(T, seed)
    vel = np.random.RandomState(100 + seed).rand(T, 88).astype(np.float32)
    return torch.from_numpy(on_p), torch.from_numpy(fr_p), torch.from_numpy(vel)


def by_public_functions(on, fr, vel, hmm, rule, m, g):
    """(pitches, intervals, velocities or None) of the existing functions.  With a model: ``extract_notes_hmm``, and for the velocities the
    documented meaning -- ``extract_notes_with_velocity`` at rule2 / 0.5 / 0.5 on the path's ONSET and ONSET-or-SUSTAIN rolls."""
    if hmm is None:
        if vel is None:
            return md.extract_notes_wo_velocity(on, fr, 0.5, 0.5, rule=rule, min_frames=m, bridge_gap=g) + (None,)
        return md.extract_notes_with_velocity(on, fr, vel, 0.5, 0.5, rule=rule, min_frames=m, bridge_gap=g)
    p, i = nh.extract_notes_hmm(on, fr, hmm, min_frames=m, bridge_gap=g)
    if vel is None:
        return p, i, None
    path_on, path_fr = nh.states_to_rolls(nh.viterbi_states(on, fr, *hmm.tables())[0])
    p2, i2, v = md.extract_notes_with_velocity(path_on, path_fr, vel, 0.5, 0.5, rule='rule2', min_frames=m, bridge_gap=g)
    assert np.array_equal(p2, p) and np.array_equal(i2, i)
    return p, i, v


def same_notes(got, want):
    for a, b in zip(got, want):
        if b is None:
            assert a is None
        else:
            assert type(a) is type(b) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def test_decoder_equals_the_public_functions():
    counts = []
    for seed, hmm, rule, (m, g), with_velocity in MATRIX:
        on, fr, vel = rolls(T, seed)
        vel = vel if with_velocity else None
        want = by_public_functions(on, fr, vel, hmm, rule, m, g)
        got = md.NoteDecoder(0.5, 0.5, rule, m, g, hmm)(on, fr, vel)
        assert len(got) == 4 and got[3] is None                         # the host side paints nothing
        same_notes(got[:3], want)
        counts.append(len(want[0]))
        if with_velocity:
            assert got[2].dtype == np.float32 and len(got[2]) == len(got[0]) and got[2].max() > 0
    print('notes per combination:', min(counts), '..', max(counts))
    assert min(counts) >= 25                                            # no combination is vacuous
    # the thresholds are the decoder's own; with a model they are unused
    on, fr, vel = rolls(T, 3)
    same_notes(md.NoteDecoder(0.3, 0.7, 'rule2')(on, fr)[:2], md.extract_notes_wo_velocity(on, fr, 0.3, 0.7, rule='rule2'))
    same_notes(md.NoteDecoder(0.9, 0.1, 'rule1', hmm=HMMS[1])(on, fr)[:2], nh.extract_notes_hmm(on, fr, HMMS[1]))
    # device tensors are no reason to leave the host: ``device`` is the caller's word alone (arrays are taken as tensors are)
    same_notes(md.NoteDecoder(rule='rule2')(on.numpy(), fr.numpy(), vel.numpy()), md.NoteDecoder(rule='rule2')(on, fr, vel))


def test_one_frame():
    for seed, hmm, rule, (m, g), with_velocity in MATRIX:
        on, fr, vel = rolls(1, seed)
        vel = vel if with_velocity else None
        got = md.NoteDecoder(0.5, 0.5, rule, m, g, hmm)(on, fr, vel)
        same_notes(got[:3], by_public_functions(on, fr, vel, hmm, rule, m, g))
        assert got[3] is None and len(got[0]) <= 88


def test_every_argument_error_is_raised_by_the_constructor():
    with pytest.raises(NameError):
        md.NoteDecoder(rule='rule3')
    for bad in (dict(min_frames=0), dict(min_frames=33), dict(bridge_gap=-1), dict(bridge_gap=32), dict(min_frames=1.5), dict(min_frames=True)):
        with pytest.raises(ValueError, match='must be an integer in'):
            md.NoteDecoder(**bad)
    with pytest.raises(TypeError, match='hmm must be a NoteHMM'):
        md.NoteDecoder(hmm=NoteHMM().tables())
    with pytest.raises(ValueError, match='use_onsets=False'):
        md.NoteDecoder(hmm=NoteHMM(), onset=False)
    md.NoteDecoder(hmm=NoteHMM(use_onsets=False), onset=False)
    md.NoteDecoder(min_frames=np.int64(32), bridge_gap=np.int32(31))
    # the device side has no fallback
    on, fr, vel = rolls(8, 3)
    for hmm in HMMS[:2]:
        with pytest.raises(RuntimeError, match='HIP device only'):
            md.NoteDecoder(hmm=hmm)(on, fr, device=True)
        with pytest.raises(RuntimeError, match='HIP device only'):
            md.NoteDecoder(hmm=hmm)(on, fr, vel, device=True)


class Counting(sc.StubModel):
    def __init__(self):
        self.calls = []

    def run_on_batch(self, label, *args):
        self.calls.append(label['path'])
        return super().run_on_batch(label, *args)


def test_one_run_on_batch_per_song():
    songs = sc.stub_songs(40, seeds=(3, 4))
    runs = {'evaluate_wo_velocity': lambda m: ev.evaluate_wo_velocity(songs, m, reconstruction=False, device_metrics=False),
            'evaluate_wo_velocity, hmm': lambda m: ev.evaluate_wo_velocity(songs, m, reconstruction=False, device_metrics=False, hmm=NoteHMM()),
            'tune_thresholds': lambda m: ev.tune_thresholds(songs, m, [0.3, 0.5], [0.5, 0.7], device_metrics=False, cleanups=[(1, 0), (2, 1)]),
            'tune_hmm': lambda m: ev.tune_hmm(songs, m, [NoteHMM(), NoteHMM(0.3, 0.7, 0.0, 1.0, 2.0)], device_metrics=False)}
    for name, run in runs.items():
        model = Counting()
        run(model)
        assert model.calls == ['stub/3', 'stub/4'], name


class TwoPassStub(sc.StubModel):
    """The posteriorgrams of the song as the result of the reconstruction pass too."""

    def run_on_batch(self, label, *args):
        pred, losses, spec = super().run_on_batch(label, *args)
        return dict(pred, onset2=pred['onset'], frame2=pred['frame']), losses, spec


def note_scores(ref, est):
    (pr, ir), (pe, ie) = ev._to_eval_units(*ref), ev._to_eval_units(*est)
    return ev.evaluate_notes(ir, pr, ie, pe, offset_ratio=None), ev.evaluate_notes(ir, pr, ie, pe)


def test_the_rules_of_the_second_pass_and_of_tune_hmm_stay():
    """The ``_2`` decode runs at the decoder's default rule1 whatever ``rule`` says (as in the reference) while the labels and the main pass
    follow ``rule``; ``tune_hmm`` decodes the labels at rule2; ``onset=False`` decodes the frame rolls alone, but the ``_2`` pass still
    reads ``onset2``."""
    song = sc.stub_songs(T, seeds=(3,))[0]
    lab, est = (song['onset'], song['frame']), (song['pred_onset'], song['pred_frame'])
    main, second = md.extract_notes_wo_velocity(*est, rule='rule2', min_frames=2), md.extract_notes_wo_velocity(*est, rule='rule1', min_frames=2)
    assert len(main[0]) != len(second[0])                               # the two rules differ on this song
    got = ev.evaluate_wo_velocity([song], TwoPassStub(), rule='rule2', reconstruction=True, device_metrics=False, min_frames=2)
    for suffix, notes in (('', main), ('_2', second)):
        plain, with_offsets = note_scores(md.extract_notes_wo_velocity(*lab, rule='rule2'), notes)
        for k, a, b in zip(('precision', 'recall', 'f1', 'overlap'), plain, with_offsets):
            assert got['metric/note/' + k + suffix] == [a] and got['metric/note-with-offsets/' + k + suffix] == [b], (suffix, k)
    # onset=False: labels from (frame, frame), estimate from (frame, frame), the second pass from (onset2, frame2) at rule1
    got = ev.evaluate_wo_velocity([song], TwoPassStub(), rule='rule2', reconstruction=True, onset=False, device_metrics=False)
    ref = md.extract_notes_wo_velocity(lab[1], lab[1], rule='rule2')
    for suffix, notes in (('', md.extract_notes_wo_velocity(est[1], est[1], rule='rule2')), ('_2', md.extract_notes_wo_velocity(*est, rule='rule1'))):
        plain, _ = note_scores(ref, notes)
        assert got['metric/note/f1' + suffix] == [plain[2]] and plain[2] > 0, suffix
    # tune_hmm: labels at rule2 -- a label whose onset has no frame under it is a note at rule2 only
    on_r, fr_r = song['onset'].clone(), song['frame'].clone()
    free = [(t, p) for t in range(5, T - 5, 10) for p in (0, 87) if fr_r[t - 2:t + 3, p].sum() == 0 and on_r[t - 2:t + 3, p].sum() == 0][:4]
    for t, p in free:
        on_r[t, p] = 1.0
    lonely = dict(song, onset=on_r, frame=fr_r)
    n1, n2 = (len(md.extract_notes_wo_velocity(on_r, fr_r, rule=r)[0]) for r in RULES)
    assert len(free) == 4 and n2 == n1 + 4
    h = NoteHMM()
    plain, _ = note_scores(md.extract_notes_wo_velocity(on_r, fr_r, rule='rule2'), nh.extract_notes_hmm(*est, h))
    res = ev.tune_hmm([lonely], sc.StubModel(), [h], device_metrics=False)
    assert res['values']['note_recall'][0] == plain[1] > 0
