"""match_notes_sparse (the note matcher of the device evaluation path) against match_notes: the identical pair list,
which needs the identical CSR graph, not merely a matching of the same size.  Runs on the CPU."""
import tracemalloc

import numpy as np

from reconvat_amd import evaluate as ev
from reconvat_amd.constants import HOP_LENGTH, SAMPLE_RATE, MIN_MIDI


def jittered_notes(n, seed, frames_per_note=8):
    """n reference notes on the frame grid and estimates derived from them: onset and offset moved by -2..+2 frames, one pitch in
    eight changed, one note in ten duplicated (so that maximum matchings are not unique), a few dropped.  Reference durations
    include 5, 10 and 15 frames, where 0.2 * duration is a whole number of hops in exact arithmetic and the float64 comparison of
    match_notes decides.  Returned in evaluation units (seconds, Hz), as evaluate_wo_velocity passes them."""
    rng = np.random.RandomState(seed)
    onset = np.sort(rng.randint(0, n * frames_per_note, size=n))
    dur = rng.choice([1, 2, 3, 5, 10, 15, 25, 40], size=n)
    ref_i = np.stack([onset, onset + dur], axis=1)
    ref_p = rng.randint(0, 88, size=n)
    est_i = ref_i + rng.randint(-2, 3, size=(n, 2))
    est_i[:, 0] = np.maximum(est_i[:, 0], 0)
    est_i[:, 1] = np.maximum(est_i[:, 1], est_i[:, 0] + 1)
    est_p = np.where(rng.rand(n) < 0.125, rng.randint(0, 88, size=n), ref_p)
    dup = rng.rand(n) < 0.1
    est_i = np.concatenate([est_i, est_i[dup] + rng.randint(-1, 2, size=(dup.sum(), 2))])
    est_i[:, 1] = np.maximum(est_i[:, 1], est_i[:, 0] + 1)
    est_p = np.concatenate([est_p, est_p[dup]])
    keep = rng.rand(len(est_p)) > 0.05
    est_i, est_p = est_i[keep], est_p[keep]
    order = np.lexsort((est_p, est_i[:, 0]))                           # the decoder's (t, pitch) order
    est_i, est_p = est_i[order], est_p[order]
    scaling = HOP_LENGTH / SAMPLE_RATE
    hz = lambda p: ev.midi_to_hz(MIN_MIDI + p)
    return ref_i * scaling, hz(ref_p), est_i * scaling, hz(est_p)


def test_sparse_matching_returns_the_pairs_of_the_dense_route():
    for seed in (0, 1, 2):
        ref_i, ref_p, est_i, est_p = jittered_notes(400, seed)
        for offset_ratio in (None, 0.2):
            want = ev.match_notes(ref_i, ref_p, est_i, est_p, offset_ratio=offset_ratio)
            got = ev.match_notes_sparse(ref_i, ref_p, est_i, est_p, offset_ratio=offset_ratio)
            assert 100 < len(want) < 400                               # the case is neither trivial nor perfect
            assert got == want, (seed, offset_ratio)
    # the duplicates make some reference note compete for more than one estimate
    ref_i, ref_p, est_i, est_p = jittered_notes(400, 0)
    d = np.abs(np.subtract.outer(ref_i[:, 0], est_i[:, 0])) <= 0.05
    d &= np.abs(np.subtract.outer(np.log2(ref_p), np.log2(est_p))) < 1e-9
    assert (d.sum(axis=1) > 1).sum() > 10


def test_sparse_matching_off_the_frame_grid_and_other_tolerances():
    """The candidate window is derived from the tolerance, not from the hop: arbitrary times and a wider tolerance agree too."""
    rng = np.random.RandomState(7)
    ref_on = np.sort(rng.uniform(0, 30, size=300))
    ref_i = np.stack([ref_on, ref_on + rng.uniform(0.05, 1.0, size=300)], axis=1)
    ref_p = ev.midi_to_hz(rng.randint(40, 60, size=300))
    est_i = ref_i + rng.uniform(-0.12, 0.12, size=(300, 2))
    est_i[:, 1] = np.maximum(est_i[:, 1], est_i[:, 0] + 0.01)
    est_p = ref_p * 2.0 ** (rng.uniform(-80, 80, size=300) / 1200.0)
    for kw in ({}, {'offset_ratio': None}, {'onset_tolerance': 0.1, 'pitch_tolerance': 30.0}):
        assert ev.match_notes_sparse(ref_i, ref_p, est_i, est_p, **kw) == ev.match_notes(ref_i, ref_p, est_i, est_p, **kw)


def test_sparse_matching_empty_inputs():
    ref_i, ref_p, est_i, est_p = jittered_notes(20, 3)
    none_i, none_p = np.zeros((0, 2)), np.array([])
    assert ev.match_notes_sparse(none_i, none_p, est_i, est_p) == []
    assert ev.match_notes_sparse(ref_i, ref_p, none_i, none_p) == []
    assert ev.match_notes_sparse(none_i, none_p, none_i, none_p) == []
    assert ev.match_notes_sparse(np.array([]), none_p, est_i, est_p) == []      # what _to_eval_units makes of "no notes"
    # nothing within tolerance: an all-zero graph, like the dense route's
    far_i = ref_i + 100.0
    assert ev.match_notes_sparse(ref_i, ref_p, far_i, ref_p) == ev.match_notes(ref_i, ref_p, far_i, ref_p) == []
    # evaluate_notes takes the matcher
    assert ev.evaluate_notes(ref_i, ref_p, est_i, est_p, match=ev.match_notes_sparse) == ev.evaluate_notes(ref_i, ref_p, est_i, est_p)


def test_sparse_matching_allocates_no_dense_matrix():
    """6 000 x 6 000 notes (a 10-minute song): one dense float64 matrix of the host route is 288 MB; the sparse route stays far
    below that -- a condition on its memory, not a benchmark."""
    ref_i, ref_p, est_i, est_p = jittered_notes(6000, 4, frames_per_note=3)
    assert len(ref_p) == 6000 and len(est_p) > 5900
    tracemalloc.start()
    try:
        pairs = ev.match_notes_sparse(ref_i, ref_p, est_i, est_p)
        _, peak = tracemalloc.get_traced_memory()
    finally:
        tracemalloc.stop()
    assert len(pairs) > 2000
    assert peak < 200e6, peak


def test_average_precision_matches_sklearn_on_the_host():
    """average_precision_device runs wherever its tensors are; on CPU tensors it must already agree with scikit-learn (bound: see
    tests/test_eval_device_gpu.py::test_average_precision_vs_sklearn)."""
    import torch
    from sklearn.metrics import average_precision_score
    rng = np.random.RandomState(11)
    y = (rng.rand(300 * 88) < 0.1).astype(np.float32)
    for score in (rng.rand(300 * 88).astype(np.float32), (np.floor(rng.rand(300 * 88) * 16) / 16).astype(np.float32)):
        score = np.where(y > 0, np.minimum(score + 0.25, 1.0), score).astype(np.float32)
        got = ev.average_precision_device(torch.from_numpy(y), torch.from_numpy(score))
        assert abs(got - average_precision_score(y, score)) <= 1e-9
    assert ev.average_precision_device(torch.zeros(50), torch.rand(50)) == 0.0      # no positive label


def test_device_path_refuses_cpu_tensors():
    import pytest
    import torch
    from reconvat_amd import decoding
    roll = torch.zeros(10, 88)
    with pytest.raises(RuntimeError, match='HIP device only'):
        decoding.extract_notes_wo_velocity_device(roll, roll)
    with pytest.raises(RuntimeError, match='HIP device only'):
        ev.evaluate_frames_device(roll.to(torch.uint8), roll.to(torch.uint8))
    with pytest.raises(NameError):
        decoding.extract_notes_wo_velocity_device(roll, roll, rule='rule3')
