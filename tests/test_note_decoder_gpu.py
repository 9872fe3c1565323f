"""decoding.NoteDecoder with ``device=True`` against ``device=False`` on the matrix of tests/test_note_decoder.py, and the launches of
whole-song evaluation on the device, which the refactoring of evaluate.py around one decoder and one per-song pass must not change."""
import numpy as np
import pytest
import torch

import sweep_cases as sc
from test_eval_device_gpu import painted_by_host
from test_note_decoder import MATRIX, T, rolls, same_notes

pytestmark = pytest.mark.gpu


def test_device_equals_host(dev):
    from reconvat_amd import decoding as md
    for seed, hmm, rule, (m, g), with_velocity in MATRIX:
        on, fr, vel = rolls(T, seed)
        vel = vel if with_velocity else None
        decode = md.NoteDecoder(0.5, 0.5, rule, m, g, hmm)
        want = decode(on, fr, vel)
        got = decode(on.to(dev), fr.to(dev), None if vel is None else vel.to(dev), device=True)
        case = (seed, hmm, rule, m, g, with_velocity)
        assert len(want[0]) >= 25, case
        same_notes(got[:3], want[:3])
        painted = got[3]
        assert painted.is_cuda and painted.dtype == torch.uint8 and tuple(painted.shape) == (T, 88), case
        assert np.array_equal(painted.cpu().numpy(), painted_by_host(want[0], want[1], (T, 88))), case
    # device tensors, host functions: ``device`` is the caller's word, not the tensors'
    on, fr, vel = (x.to(dev) for x in rolls(T, 3))
    got = md.NoteDecoder(rule='rule2')(on, fr, vel)
    assert got[3] is None
    same_notes(got[:3], md.NoteDecoder(rule='rule2')(on.cpu(), fr.cpu(), vel.cpu())[:3])


# recorded from the commit before the refactoring, per song at T = 130: the labels' decode, the estimate's decode, the frame counters
# (AP and the note matching make no launch of the library)
LAUNCHES_PER_SONG = ['rv_eval_decode_clean', 'rv_eval_decode_clean', 'rv_eval_frame_counts']
LAUNCHES_PER_SONG_HMM = ['rv_eval_decode_clean', 'rv_hmm_decode', 'rv_eval_decode_clean', 'rv_eval_frame_counts']


def test_launches_per_song_are_those_of_the_parent(dev):
    from reconvat_amd import NoteHMM, _lib, evaluate as ev
    songs = sc.stub_songs(T, seeds=(3,), device=dev)
    names = []

    def hook(name, args, fn):
        names.append(name)
        return fn(*args)
    for hmm, want in ((None, LAUNCHES_PER_SONG), (NoteHMM(), LAUNCHES_PER_SONG_HMM)):
        del names[:]
        _lib.HOOK[0] = hook
        try:
            ev.evaluate_wo_velocity(songs, sc.StubModel(), reconstruction=False, device_metrics=True, hmm=hmm)
        finally:
            _lib.HOOK[0] = None
        assert names == want, hmm
