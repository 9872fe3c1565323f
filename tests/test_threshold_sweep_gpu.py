"""rv_eval_sweep (csrc/eval.hip) against sweep_counts_host: every comparison is == on integers.  Sizes around the
64-frame tile, both rules, aliased rolls, values exactly on a threshold, a chain that a wrong matcher fails, runs across whole
tiles, the durations at which the offset test is decided by float64 rounding, degenerate grids, repeatability, tune_thresholds
end to end, and the argument checks."""
import numpy as np
import pytest
import torch

import sweep_cases as sc

pytestmark = pytest.mark.gpu

GRIDS = {'1x1': ([0.5], [0.5]), '3x2': ([0.3, 0.5, 0.7], [0.5, 0.3]), '7x5': ([0.7, 0.2, 0.5, 0.3, 0.6, 0.4, 0.8], [0.3, 0.5, 0.7, 0.4, 0.6])}


def both(rolls, dev, on_thr, fr_thr, rule='rule2', alias=False):
    from reconvat_amd import evaluate as ev
    cpu = [torch.from_numpy(r) for r in rolls]
    gpu = [x.to(dev) for x in cpu]
    if alias:                                                          # onset=False: the frame rolls serve as onset rolls too
        cpu, gpu = [cpu[1], cpu[1], cpu[3], cpu[3]], [gpu[1], gpu[1], gpu[3], gpu[3]]
    want = ev.sweep_counts_host(*cpu, on_thr, fr_thr, rule=rule)
    got = ev.sweep_counts_device(*gpu, on_thr, fr_thr, rule=rule)
    assert set(got) == set(want)
    for k in ev.SWEEP_KEYS:
        assert got[k].dtype == np.int64 and got[k].shape == (len(on_thr), len(fr_thr))
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert got['n_ref'] == want['n_ref'] and got['frame_ref'] == want['frame_ref']
    return want


@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 129, 200])
@pytest.mark.parametrize('grid', ['1x1', '3x2', '7x5'])
def test_sizes_and_grids(dev, T, grid):
    rolls = sc.random_rolls(T, seed=100 + T, density=0.12)
    for rule in ('rule1', 'rule2'):
        both(rolls, dev, *GRIDS[grid], rule=rule)
    if grid == '3x2':
        both(rolls, dev, *GRIDS[grid], alias=True)


def test_random_rolls_exercise_the_matcher(dev):
    """Seed chosen on the CPU so that the host counters show a partial matching and offsets that remove matches."""
    on_thr, fr_thr = GRIDS['3x2']
    rolls = sc.random_rolls(200, seed=5, density=0.12)
    assert sum(int((r == np.float32(0.5)).sum()) for r in rolls[2:]) > 50      # values exactly on a threshold are in there
    want = both(rolls, dev, on_thr, fr_thr)
    m, mo, n_est = want['matched'], want['matched_with_offsets'], want['n_est']
    assert np.any((m > 0) & (m < np.minimum(want['n_ref'], n_est)))
    assert np.any(mo < m)
    both(rolls, dev, on_thr, fr_thr, rule='rule1')


def test_chain(dev):
    want = both(sc.chain_rolls(), dev, [0.5, 0.3], [0.5])
    assert want['matched'][0, 0] > 100 and 0 < want['matched_with_offsets'][0, 0] < want['matched'][0, 0]


@pytest.mark.parametrize('T', [4 * sc.TILE, 4 * sc.TILE + 4])
def test_long_runs(dev, T):
    want = both(sc.long_run_rolls(T), dev, [0.5], [0.5, 0.9])
    assert want['n_ref'] == 3 and want['matched'][0, 0] == 3 and want['frame_tp'][0, 0] > 3 * 3 * sc.TILE


def test_offset_boundary(dev):
    """Reference durations at which 0.2 * duration is a whole number of hops (5, 10, 15) and their neighbours; estimate ends 0..4
    frames either way.  One note pair per call, so the hit pattern itself is compared."""
    from reconvat_amd import evaluate as ev
    pattern = {}
    for duration in (4, 5, 6, 9, 10, 11, 15):
        for delta in range(-4, 5):
            if duration + delta < 1:
                continue
            for start in (50, 0):
                rolls = sc.offset_boundary_rolls(duration, delta, start=start)
                want = both(rolls, dev, [0.5], [0.5])
                assert want['matched'][0, 0] == 1
                pattern[duration, delta, start] = int(want['matched_with_offsets'][0, 0])
    assert set(pattern.values()) == {0, 1}
    assert pattern[10, 2, 0] == 1 and pattern[10, 2, 50] == 0           # float64 decides, and differently by position
    assert ev._offset_slack(np.array([[50, 60]])).tolist() == [[1, 1]]


def test_degenerate_grids(dev):
    from reconvat_amd import evaluate as ev
    rolls = sc.random_rolls(130, seed=9, density=0.12)
    want = both(rolls, dev, [1.0], [1.0])                               # nothing above 1.0: no estimate
    assert all(int(want[k][0, 0]) == 0 for k in ev.SWEEP_KEYS) and want['n_ref'] > 0
    want = both(rolls, dev, [-1.0], [-1.0, 0.5])                        # everything on: one note per pitch, every frame painted
    assert want['n_est'][0, 0] == 88 and want['frame_est'][0, 0] == 130 * 88 and want['frame_tp'][0, 0] == want['frame_ref']
    empty = [np.zeros_like(rolls[0]), np.zeros_like(rolls[1]), rolls[2], rolls[3]]
    want = both(empty, dev, *GRIDS['3x2'])                              # labels without a note
    assert want['n_ref'] == 0 and want['frame_ref'] == 0 and not want['matched'].any() and want['n_est'].any()
    on_thr, fr_thr = [0.5, 0.3, 0.5, 0.7, 0.3], [0.6, 0.2, 0.6]        # duplicates, unsorted
    want = both(rolls, dev, on_thr, fr_thr)
    got = ev.sweep_counts_device(*[torch.from_numpy(r).to(dev) for r in rolls], on_thr, fr_thr)
    for k in ev.SWEEP_KEYS:
        assert np.array_equal(got[k][0], got[k][2]) and np.array_equal(got[k][1], got[k][4]) and np.array_equal(got[k][:, 0], got[k][:, 2])
    assert not np.array_equal(want['n_est'][0], want['n_est'][1])


def raw_call(dev, rolls, n_on=3, n_fr=2, rule=2, ws_bytes=None):
    """rv_eval_sweep called directly on valid buffers; returns (status, counts, totals)."""
    from reconvat_amd import _lib
    T = rolls[2].shape[0]
    on, fr = torch.from_numpy(rolls[2]).to(dev), torch.from_numpy(rolls[3]).to(dev)
    thr = torch.tensor([0.3, 0.5, 0.7] * 11 + [0.5, 0.3] * 17, dtype=torch.float32, device=dev)
    ref = torch.zeros((1, 5), dtype=torch.int32, device=dev)
    roll = torch.zeros((T, 88), dtype=torch.uint8, device=dev)
    need = _lib.load().rv_eval_sweep_workspace_bytes(T, 3, 2)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    counts = torch.full((32 * 32 * 5,), -7, dtype=torch.int64, device=dev)
    totals = torch.full((2,), -7, dtype=torch.int64, device=dev)
    rc = _lib.invoke('rv_eval_sweep', on.data_ptr(), fr.data_ptr(), T, thr.data_ptr(), n_on, thr.data_ptr() + 4 * 33, n_fr, rule,
                     ref.data_ptr(), 0, roll.data_ptr(), counts.data_ptr(), totals.data_ptr(), ws.data_ptr(),
                     need if ws_bytes is None else ws_bytes, _lib.stream())
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy(), totals.cpu().numpy()


def test_repeatable(dev):
    rolls = sc.random_rolls(200, seed=5, density=0.12)
    first, second = raw_call(dev, rolls), raw_call(dev, rolls)
    assert first[0] == second[0] == 0
    assert np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])
    assert first[1][:30].min() >= 0 and first[1][:30].max() > 0 and np.all(first[1][30:] == -7)      # 3 x 2 x 5 counters, no more
    from reconvat_amd import evaluate as ev
    gpu = [torch.from_numpy(r).to(dev) for r in rolls]
    a, b = ev.sweep_counts_device(*gpu, *GRIDS['7x5']), ev.sweep_counts_device(*gpu, *GRIDS['7x5'])
    assert all(np.array_equal(a[k], b[k]) for k in ev.SWEEP_KEYS)


def test_end_to_end_tuning(dev):
    from reconvat_amd import evaluate as ev
    model = sc.StubModel()
    on_thr, fr_thr = GRIDS['3x2']
    want = ev.tune_thresholds(sc.stub_songs(130, (3, 4)), model, on_thr, fr_thr, device_metrics=False)
    got = ev.tune_thresholds(sc.stub_songs(130, (3, 4), device=dev), model, on_thr, fr_thr, device_metrics=True)
    assert set(got['grid']) == set(want['grid']) and len(want['grid']) == 9
    for k in want['grid']:
        assert np.array_equal(got['grid'][k], want['grid'][k]), k
    assert got['best_index'] == want['best_index'] and got['best_value'] == want['best_value'] > 0
    assert (got['onset_threshold'], got['frame_threshold']) == (want['onset_threshold'], want['frame_threshold'])


def test_argument_errors(dev):
    from reconvat_amd import _lib, evaluate as ev
    lib = _lib.load()
    assert lib.rv_eval_sweep_workspace_bytes(200, 0, 2) == 0 and lib.rv_eval_sweep_workspace_bytes(200, 33, 2) == 0
    assert lib.rv_eval_sweep_workspace_bytes(200, 2, 0) == 0 and lib.rv_eval_sweep_workspace_bytes(200, 2, 33) == 0
    assert lib.rv_eval_sweep_workspace_bytes(0, 2, 2) == 0 and lib.rv_eval_sweep_workspace_bytes((1 << 24) + 1, 2, 2) == 0
    assert lib.rv_eval_sweep_workspace_bytes(200, 3, 2) == (2 * 3 + 2 + 1) * 4 * 88 * 8
    rolls = sc.random_rolls(200, seed=5, density=0.12)
    for kw in (dict(n_on=0), dict(n_on=33), dict(n_fr=0), dict(n_fr=33), dict(rule=3), dict(ws_bytes=(2 * 3 + 2 + 1) * 4 * 88 * 8 - 16)):
        rc, counts, totals = raw_call(dev, rolls, **kw)
        assert rc == -1, kw
        assert np.all(counts == -7) and np.all(totals == -7), kw       # nothing was launched
        assert 'rv_eval_sweep' in _lib.last_error()
    gpu = [torch.from_numpy(r).to(dev) for r in rolls]
    with pytest.raises(ValueError):
        ev.sweep_counts_device(*gpu, [], [0.5])
    with pytest.raises(ValueError):
        ev.sweep_counts_device(*gpu, [0.5] * 33, [0.5])
    with pytest.raises(NameError):
        ev.sweep_counts_device(*gpu, [0.5], [0.5], rule='rule3')
    with pytest.raises(RuntimeError, match='HIP device only'):
        ev.sweep_counts_device(*[torch.from_numpy(r) for r in rolls], [0.5], [0.5])
