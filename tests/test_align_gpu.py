"""Score-to-recording alignment on the device (rv_align_cost, rv_align_dtw) against the host definition of
reconvat_amd/align.py.  The DTW kernel's outputs are integers with a fixed tie rule: total, path length, the four path arrays and the
direction byte of every live cell EQUAL `dtw_host`'s on the same cost matrix.  The cost kernel sums in float32 on the matrix pipe: a
cell may differ from the float64 yardstick's by 1, and the share of cells that differ at all is capped at twice the share at which a
float32 NumPy evaluation of the same inputs differs (two different float32 summation orders)."""
import os

import numpy as np
import pytest
import torch

import align_cases as ac
from reconvat_amd import _lib, align

pytestmark = pytest.mark.gpu


def band_cost(rng, lo, W, M, values):
    cost = rng.choice(values, size=(len(lo), W)).astype(np.uint16)
    cost[np.asarray(lo)[:, None] + np.arange(W)[None, :] >= M] = align.DEAD
    return cost


def full_lo(N):
    return np.zeros(N, dtype=np.int32)


# ---- the cost kernel
COST_CASES = {'full 70x45 D=229': (70, 45, 229, None, 15), 'jumpy 70x200 D=230 W=33': (70, 200, 230, 33, 16)}


@pytest.mark.parametrize('case', list(COST_CASES))
def test_cost_kernel(dev, case):
    """Unit rows from a seeded generator, rounded to float32 before either evaluation.  A float32 NumPy evaluation (`cost_host` with
    dtype=float32: a float32 matrix product) differs from the float64 one only in cells whose value lies next to a rounding boundary,
    0 .. 5 of them in a draw of these sizes; the seeds are those of 11 .. 16 at which it differs in the most cells.  Measured:
         full 70 x 45, D = 229 (K tail, no dimension a multiple of 32), seed 15:  float32 NumPy differs in 5 of 3150 live cells, the kernel in 2
         jumpy 70 x 200, D = 230, W = 33, seed 16:                                float32 NumPy differs in 2 of 2152 live cells, the kernel in 1
    so the caps are 10 and 4 cells.  The figures are printed before the assertions (DESIGN 3.16 records them)."""
    N, M, D, W, seed = COST_CASES[case]
    rng = np.random.RandomState(seed)
    X, Y = ac.unit_rows(rng, N, D).astype(np.float32), ac.unit_rows(rng, M, D).astype(np.float32)
    lo, W = (full_lo(N), M) if W is None else (ac.jumpy_lo(N, M, W), W)
    want = align.cost_host(X, Y, lo, W)                                      # float64 on the same float32 inputs
    f32 = align.cost_host(X, Y, lo, W, dtype=np.float32)
    live = want != align.DEAD
    share32 = float((f32 != want)[live].mean())
    flat, lay = align.cost_device([(X, Y)], [lo], [W], dev)
    got = flat.cpu().numpy().view(np.uint16).reshape(N, W)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    share = float((diff != 0)[live].mean())
    print(f'{case}: {int(live.sum())} live cells; float32 NumPy differs in {int((f32 != want)[live].sum())} ({share32:.4%}), '
          f'the kernel in {int((diff != 0)[live].sum())} ({share:.4%}), largest difference {int(diff[live].max())}')
    assert share32 > 0                                                       # the cap is not vacuous
    assert (got[~live] == align.DEAD).all() and (want[~live] == align.DEAD).all()
    assert diff[live].max() <= 1
    assert share <= 2 * share32


def test_cost_kernel_batch_and_guards(dev):
    """Three pairs in one launch give the cells of three single launches; a table row that does not fit its buffers is left alone."""
    rng = np.random.RandomState(12)
    shapes = [(33, 40, None), (70, 200, 33), (5, 64, 17)]
    pairs, los, Ws = [], [], []
    for N, M, W in shapes:
        pairs.append((ac.unit_rows(rng, N, 19).astype(np.float32), ac.unit_rows(rng, M, 19).astype(np.float32)))
        los.append(full_lo(N) if W is None else (ac.jumpy_lo(N, M, W) if N == 70 else np.minimum(np.arange(N) * 11, M - W).astype(np.int32)))
        Ws.append(M if W is None else W)
    flat, lay = align.cost_device(pairs, los, Ws, dev)
    parts = lay.split_cells(flat.cpu().numpy().view(np.uint16))
    for p in range(3):
        single, _ = align.cost_device([pairs[p]], [los[p]], [Ws[p]], dev)
        assert np.array_equal(parts[p], single.cpu().numpy().view(np.uint16).reshape(parts[p].shape))
        assert np.abs(parts[p].astype(np.int64) - align.cost_host(*pairs[p], los[p], Ws[p]).astype(np.int64)).max() <= 1
    # the same launch with a cost buffer declared one cell short of the last pair: that pair is skipped, the others are written
    from reconvat_amd._lib import ptr
    feats = torch.cat([torch.from_numpy(a).reshape(-1) for x, y in pairs for a in (x, y)]).to(dev)
    lo = torch.from_numpy(np.concatenate(los).astype(np.int32)).to(dev)
    desc = torch.from_numpy(lay.table).to(dev)
    cost = torch.full((lay.n_cells,), 0x5555, dtype=torch.int16, device=dev)
    lib = _lib.load()
    assert lib.rv_align_cost(ptr(desc), 3, 19, lay.max_n, lay.max_w, ptr(feats), feats.numel(), ptr(lo), lo.numel(), ptr(cost), lay.n_cells - 1, None) == 0
    torch.cuda.synchronize()
    again = lay.split_cells(cost.cpu().numpy().view(np.uint16))
    assert np.array_equal(again[0], parts[0]) and np.array_equal(again[1], parts[1]) and (again[2] == 0x5555).all()
    for bad, rc in (((ptr(desc), 3, 19, lay.max_n, 8193), -3), ((ptr(desc), 0, 19, lay.max_n, lay.max_w), -1),
                    ((ptr(desc), 3, 0, lay.max_n, lay.max_w), -1), ((None, 3, 19, lay.max_n, lay.max_w), -1)):
        assert lib.rv_align_cost(*bad, ptr(feats), feats.numel(), ptr(lo), lo.numel(), ptr(cost), lay.n_cells, None) == rc
        assert 'rv_align_cost' in _lib.last_error()


# ---- the DTW kernel: exact equality on cost matrices made on the host
def dtw_case(name):
    rng = np.random.RandomState(sum(map(ord, name)))
    if name.startswith('tiny'):
        N, M = {'tiny 1x1': (1, 1), 'tiny 1x7': (1, 7), 'tiny 9x1': (9, 1), 'tiny 13x11': (13, 11)}[name]
        return band_cost(rng, full_lo(N), M, M, [0, 1, 2]), full_lo(N), M, M
    if name in ('ties 64x64', 'ties 65x63'):
        N, M = (64, 64) if name.endswith('64') else (65, 63)
        return band_cost(rng, full_lo(N), M, M, [0, 1]), full_lo(N), M, M
    if name == 'all 4095 300x300':
        return np.full((300, 300), 4095, dtype=np.uint16), full_lo(300), 300, 300
    if name == 'full 1500x1500':
        return rng.randint(0, 4096, size=(1500, 1500)).astype(np.uint16), full_lo(1500), 1500, 1500
    if name == 'narrow 3000x3000 W=5':
        lo = np.clip(np.arange(3000) - 2, 0, 3000 - 5).astype(np.int32)
        return band_cost(rng, lo, 5, 3000, [0, 1, 2, 4095]), lo, 5, 3000
    if name == 'jumpy 70x200 W=33':
        lo = ac.jumpy_lo()
        return band_cost(rng, lo, 33, 200, [0, 1, 2]), lo, 33, 200
    if name == 'widest band 3x8192':                                         # three rings of 8193 words: past 64 KiB of LDS
        return band_cost(rng, full_lo(3), 8192, 8192, [0, 1, 2]), full_lo(3), 8192, 8192
    if name == 'disconnected':
        lo = np.array([0, 0, 0, 8, 8, 9], dtype=np.int32)
        return band_cost(rng, lo, 3, 12, [1, 2]), lo, 3, 12
    raise KeyError(name)


DTW_CASES = ['tiny 1x1', 'tiny 1x7', 'tiny 9x1', 'tiny 13x11', 'ties 64x64', 'ties 65x63', 'all 4095 300x300', 'full 1500x1500',
             'narrow 3000x3000 W=5', 'jumpy 70x200 W=33', 'widest band 3x8192', 'disconnected']


@pytest.mark.parametrize('name', DTW_CASES)
def test_dtw_kernel_equals_the_host(dev, name):
    cost, lo, W, M = dtw_case(name)
    want = align.dtw_host(cost, lo, W, M)
    got = align.dtw_device([cost], [lo], [W], [M], dev, keep_dirs=True)[0]
    live = cost != align.DEAD                                                # reachable cells and more: an unreachable live cell holds 3 on both sides
    ac.same_result(got, want, dirs_where=live)
    assert (got['dirs'][~live] == 3).all()                                   # dead cells are not written
    if name == 'disconnected':
        assert got['total'] == align.SENTINEL and got['length'] == 0 and (got['row_lo'] == -1).all() and (got['col_hi'] == -1).all()
    else:
        assert got['total'] < 1 << 30 and got['length'] >= max(len(lo), M)
    if name == 'all 4095 300x300':
        assert got['total'] == 4095 * 600
    if name.startswith('tiny'):
        ac.check_result(got, cost, lo, W, M)                                 # and against the plain double loop itself


def test_dtw_kernel_batch_equals_single_calls(dev):
    names = ['ties 65x63', 'jumpy 70x200 W=33', 'tiny 9x1']
    cases = [dtw_case(n) for n in names]
    batch = align.dtw_device([c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], dev, keep_dirs=True)
    for (cost, lo, W, M), res in zip(cases, batch):
        single = align.dtw_device([cost], [lo], [W], [M], dev, keep_dirs=True)[0]
        live = cost != align.DEAD
        ac.same_result(res, single, dirs_where=live)
        ac.same_result(res, align.dtw_host(cost, lo, W, M), dirs_where=live)


def test_dtw_kernel_guards(dev):
    """Sizes past the limits are refused with -3 before a launch; a table row that does not fit its buffers gets status -1 and nothing else."""
    from reconvat_amd._lib import ptr
    cost, lo, W, M = dtw_case('tiny 13x11')
    lay = align._Layout([13], [M], [W])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    desc, lo_d, cost_d = d(lay.table), d(lo), d(cost.view(np.int16).reshape(-1))
    dirs = torch.full((lay.n_cells,), 7, dtype=torch.uint8, device=dev)
    out = torch.full((lay.n_out,), 99, dtype=torch.int32, device=dev)
    lib = _lib.load()
    tail = (ptr(lo_d), 13, ptr(cost_d), lay.n_cells, ptr(dirs), lay.n_cells, ptr(out))
    assert lib.rv_align_dtw(ptr(desc), 1, (1 << 18) + 1, W, *tail, lay.n_out, None) == -3 and '2^18' in _lib.last_error()
    assert lib.rv_align_dtw(ptr(desc), 1, 13 + M, 8193, *tail, lay.n_out, None) == -3
    assert lib.rv_align_dtw(ptr(desc), 0, 13 + M, W, *tail, lay.n_out, None) == -1
    assert lib.rv_align_dtw(ptr(desc), 1, 13 + M, W, *tail, lay.n_out - 1, None) == 0       # the output declared one word short
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert o[2] == -1 and np.uint32(o[0]) == align.SENTINEL and o[1] == 0 and (o[4:] == 99).all() and (dirs.cpu().numpy() == 7).all()
    assert lib.rv_align_dtw(ptr(desc), 1, 13 + M - 1, W, *tail, lay.n_out, None) == 0       # N + M above the declared bound
    torch.cuda.synchronize()
    assert out.cpu().numpy()[2] == -1 and (dirs.cpu().numpy() == 7).all()
    with pytest.raises(ValueError, match=r'2\^18'):
        align.dtw_device([np.broadcast_to(np.zeros((1, 1), dtype=np.uint16), (1 << 18, 1))], [np.zeros(1 << 18, dtype=np.int32)], [1], [5], dev)


# ---- end to end
def test_end_to_end_on_the_device(dev):
    """The 12 s case of tests/test_align.py through align_score(device='cuda').  Each side's path is priced by the other side's cost
    matrix, whose cells differ by at most 1 and are counted at most twice: |total_dev - total_host| <= 2 (N + M - 1)."""
    notes, rec, truth = ac.e2e_case()
    host, host_report = align.align_score(rec, notes, device='cpu')
    got, report = align.align_score(rec, notes, device=dev)
    N, M = report['N'], report['M']
    share, share_host = ac.onset_share(got, truth), ac.onset_share(host, truth)
    print(f'device: total {report["total"]}, {share:.3f} of {len(notes)} onsets within 50 ms; host: total {host_report["total"]}, {share_host:.3f}')
    assert (N, M, report['S'], report['W']) == (host_report['N'], host_report['M'], host_report['S'], host_report['W'])
    assert abs(report['total'] - host_report['total']) <= 2 * (N + M - 1)
    assert share >= 0.90 and share_host >= 0.90
    assert np.array_equal(got[:, 2:], notes[:, 2:])


def test_align_scores_cli_on_the_device(dev, tmp_path):
    import align_scores
    from reconvat_amd.dataset import read_audio_int16
    folder = str(tmp_path)
    scores = ac.make_folder(folder)
    done = align_scores.main(['with', f'input={folder}', f'device={dev}'])
    assert [d[0] for d in done] == [f'piece{i}' for i in range(5)] and not os.path.exists(os.path.join(folder, 'piece5.tsv'))
    for name, target, report in done:
        rows = np.loadtxt(target, delimiter='\t', skiprows=1, ndmin=2)
        direct, direct_report = align.align_score(read_audio_int16(os.path.join(folder, name + '.wav')), scores[name], device=dev)
        assert np.allclose(rows, direct, atol=1e-6) and report == direct_report
