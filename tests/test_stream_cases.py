"""CPU checks of tests/stream_cases.py: every case sits in the launch regime it is labelled with, the float32 CPU reference alone
meets the tolerances the GPU tests apply (no case is born failing), and each outlier moves its result by >= 10x the tolerance."""
import pytest
import torch
import torch.nn.functional as F

import stream_cases as sc


def _in_regime(launch, regime):
    for k, v in regime.items():
        assert launch[k] == v, (k, launch[k], v, launch)


@pytest.mark.parametrize('case', list(sc.BN_CASES), ids=sc.bn_id)
def test_bn_case_reaches_its_regime(case):
    C, P = case
    red, fwd, bwd = sc.BN_CASES[case]
    _in_regime(sc.bn_reduce_launch(P, C), red)
    _in_regime(sc.bn_apply_launch(P, C, False), fwd)
    _in_regime(sc.bn_apply_launch(P, C, True), bwd)


def test_bn_case_table_covers_the_regimes():
    """between them the cases reach: ppt above its floor, all replicas and the wrap, both apply loops, a capped grid in each loop,
    more than one trip forward and backward, the LDS fold at PL = 256, idle reduction threads"""
    red = [sc.bn_reduce_launch(P, C) for C, P in sc.BN_CASES]
    fwd = [sc.bn_apply_launch(P, C, False) for C, P in sc.BN_CASES]
    bwd = [sc.bn_apply_launch(P, C, True) for C, P in sc.BN_CASES]
    assert any(r['ppt'] > sc.BN_PIX_PER_THREAD for r in red) and any(r['replica_wrap'] for r in red)
    assert any(r['replicas'] == sc.RV_BN_NREP and r['reduce_masked_tail'] for r in red)
    assert any(r['PL'] == 256 for r in red) and any(r['idle_threads'] for r in red)
    assert any(a['fixed'] and a['trips'] > 1 for a in fwd) and any(a['fixed'] and a['trips'] > 2 for a in bwd)
    assert any(not a['fixed'] and a['passes'] > 1 and a['apply_blocks'] == sc.BN_MAXBLK for a in fwd)
    assert any(not a['fixed'] and a['passes'] == 1 for a in fwd)
    # the shapes the older tests run stay in the trivial regime -- which is why this table exists
    r0, a0 = sc.bn_reduce_launch(182, 16), sc.bn_apply_launch(2736, 32, False)
    assert r0['reduce_blocks'] == 1 and r0['ppt'] == 16 and a0['pixels_per_thread'] == 1


def test_colsum_and_reduction_cases_reach_their_regimes():
    for M, N, ld, off, regime in sc.COLSUM_CASES:
        _in_regime(sc.colsum_path(N, ld, M, aligned16=off % 4 == 0), regime)
    assert {sc.colsum_path(N, ld, M, off % 4 == 0)['path'] for M, N, ld, off, _ in sc.COLSUM_CASES} == {'vec', 'generic'}
    assert sc.colsum_path(88, 88, 1025)['path'] == 'vec'              # ... so M = 1023 and the offset pointer are what move N = 88
    for M, N, regime in sc.COLSUM_ORDERED_CASES:
        _in_regime(sc.colsum_ordered_launch(M, N), regime)
    for n, (regime, _) in sc.REDUCE_CASES.items():
        _in_regime(sc.reduce_parts(n), regime)
    assert [sc.grid_stride_passes(n) for n in sc.GRID_STRIDE_N] == [1, 2]
    M, N = sc.SIGMOID_BWD_CASES[-1]
    assert M * N == 1048576 + 88 and sc.grid_stride_passes(M * N) == 2


def _bn_modes(case):
    yield case, True, None
    yield case, False, None
    if case in sc.BN_OPTION_CASES:
        for r in sc.BN_R[:2]:
            yield case, True, r


@pytest.mark.parametrize('case', list(sc.BN_CASES), ids=sc.bn_id)
def test_bn_float32_reference_meets_the_tolerances(case):
    """torch's float32 CPU batch_norm + leaky_relu and autograd against bn_reference, under the checks of the GPU test"""
    for (C, P), training, r in _bn_modes(case):
        pr = sc.bn_problem(C, P, training, r)
        ref = sc.bn_reference(pr, training)
        body = ref['zh'][1:P - 1]
        assert P <= 2 or body.abs().min().item() > sc.KINK_GUARD, 'an element sits on the leaky-ReLU kink'
        z, gamma, beta = (pr[k].clone().requires_grad_(True) for k in ('z', 'gamma', 'beta'))
        rm, rv = pr['rm'].clone(), pr['rv'].clone()
        y = F.leaky_relu(F.batch_norm(z.t()[None], rm, rv, gamma, beta, training, sc.MOMENTUM, sc.EPS), sc.SLOPE)[0].t()
        (y * pr['dy']).sum().backward()
        where = f'{sc.bn_id(case)} training={training} r={r}'
        for key, got, want, tol, terms in (('y', y, ref['y'], sc.TOL, None), ('dz', z.grad, ref['dz'], sc.TOL_G, ref['dz_terms'])):
            b, rows = sc.body_and_rows(got, want, terms)
            sc.check(where, 'cpu-f32', key, b, tol)
            sc.check(where, 'cpu-f32', key + ' outlier rows', rows, tol)
        sc.check(where, 'cpu-f32', 'dgamma', sc.max_rel(gamma.grad, ref['dgamma']), sc.TOL_G)
        sc.check(where, 'cpu-f32', 'dbeta', sc.max_rel(beta.grad, ref['dbeta']), sc.TOL_G)
        if training:
            for k, (e, t) in sc.bn_running_errors(rm, rv, ref).items():
                sc.check(where, 'cpu-f32', k, e, t)
            mean = pr['z'].mean(0)
            var = pr['z'].var(0, unbiased=False)
            got5 = torch.stack([mean, 1 / torch.sqrt(var + sc.EPS), pr['gamma'] / torch.sqrt(var + sc.EPS),
                                pr['beta'] - mean * pr['gamma'] / torch.sqrt(var + sc.EPS), var * P / (P - 1)])
            for k, (e, t) in sc.bn_coef_errors(got5, ref, True).items():
                sc.check(where, 'cpu-f32', k, e, t)


@pytest.mark.parametrize('case', list(sc.BN_CASES), ids=sc.bn_id)
def test_bn_outlier_rows_move_every_reduction_by_ten_tolerances(case):
    C, P = case
    for r in (None, 10):
        pr = sc.bn_problem(C, P, True, r)
        ref = sc.bn_reference(pr, True)
        z, std = pr['z'].double(), torch.sqrt(ref['var'])
        mean = ref['coef'][0]
        for row in (0, P - 1):
            # a dropped (or, for row 0, double-counted) row moves the batch mean by |z - mean| / P
            assert (((z[row] - mean).abs() / P) / (sc.TOL_STAT * std)).min().item() >= 10, (case, row)
            assert sc.OUTLIER / P >= 10 * sc.TOL_STAT * std.max().item()
            # ... the variance by about (z - mean)^2 / P, invstd by half of that relatively
            if P > 2:                                                # (of two rows, either one IS half the variance)
                assert ((((z[row] - mean) ** 2 - ref['var']).abs() / P / ref['var']) / max(sc.TOL_STAT, 2 * sc.TOL_INVSTD)).min().item() >= 10
            # ... dbeta by dd[row], dgamma by dd[row] * xhat[row]: in the channels where the activation passes the outlier
            xh = (z[row] - mean) * ref['coef'][1]
            assert (ref['dd'][row].abs().max() / (sc.TOL_G * ref['dbeta'].abs().max())).item() >= 10, (case, row)
            assert ((ref['dd'][row] * xh).abs().max() / (sc.TOL_G * ref['dgamma'].abs().max())).item() >= 10, (case, row)


def test_colsum_float32_reference_and_outliers():
    for M, N, ld, off, _ in sc.COLSUM_CASES + [(M, N, N, 0, None) for M, N, _ in sc.COLSUM_ORDERED_CASES]:
        x = sc.colsum_view(sc.colsum_input(M, N, ld, off), M, N, ld, off)
        ref = x.double().sum(0)
        s = torch.zeros(N)
        for blk in x.split(256):                                     # float32 all the way, folded block by block
            s += blk.sum(0)
        sc.check('colsum', f'{M}x{N}', 'cpu-f32', sc.max_rel(s, ref), sc.TOL_COLSUM)
        for row in (0, M - 1):
            assert ((x[row].double() - 0.5).abs().min() / (sc.TOL_COLSUM * ref.abs().max())).item() >= 10, (M, N, row)


@pytest.mark.parametrize('kind', list(sc.REDUCE_KINDS))
def test_reduce_float32_reference_and_outliers(kind):
    for n, (_, amp) in sc.REDUCE_CASES.items():
        p, t = sc.reduce_input(kind, n, amp)
        ref = sc.reduce_reference(kind, p, t)
        got = {'bce': lambda: -(t * p.log().clamp_min(-100) + (1 - t) * (1 - p).log().clamp_min(-100)).mean(),   # (the outlier's target is > 1)
                'mse': lambda: F.mse_loss(p, t), 'abs': lambda: p.abs().mean(),
               'l2': lambda: p.norm()}[kind]()
        sc.check('reduce', f'{kind} n={n}', 'cpu-f32', abs(got.item() - ref.item()) / abs(ref.item()), sc.TOL)
        assert sc.reduce_drop_shift(kind, p, t) >= 10 * sc.TOL, (kind, n, sc.reduce_drop_shift(kind, p, t))


def test_elementwise_float32_references():
    for n in sc.GRID_STRIDE_N:
        for kind in ('bce', 'mse'):
            p, t = sc.loss_bwd_input(kind, n)
            pr = p.clone().requires_grad_(True)
            (1.7 * (F.binary_cross_entropy(pr, t) if kind == 'bce' else F.mse_loss(pr, t))).backward()
            ref = sc.loss_bwd_reference(kind, p, t, 1.7)
            sc.check('loss_bwd', f'{kind} n={n}', 'cpu-f32 body', sc.max_rel(pr.grad[2:], ref[2:]), sc.TOL_G)
            sc.check('loss_bwd', f'{kind} n={n}', 'cpu-f32 clamped', ((pr.grad[:2].double() - ref[:2]).abs() / ref[:2].abs()).max().item(), sc.TOL_G)
    # Adam: torch.optim.Adam in float32 under StepLR against the float64 restatement
    n = 1000
    g = sc._gen(n, 5)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (k + 1) for k in range(3)]
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], 1e-3)
    sch = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)
    for gk in grads:
        q.grad = gk * 0.5
        opt.step()
        sch.step()
    ref, _, _ = sc.adam_reference(p0, grads, 1e-3, 2, 0.5, 0.9, 0.999, 1e-8, 0.5)
    sc.check('adam', 'n=1000', 'cpu-f32', sc.max_rel(q, ref), sc.TOL_ADAM)
    # VAT perturbation: torch float32 autograd against vat_reference
    for rows in sc.VAT_ROWS:
        for n in sc.VAT_N:
            for xi in sc.VAT_XI:
                x, d, cot = sc.vat_input(rows, n)
                dr = d.clone().requires_grad_(True)
                xa = (x + xi * dr / torch.norm(dr, dim=-1, keepdim=True)).clamp(0, 1)
                (xa * cot).sum().backward()
                ref = sc.vat_reference(x, d, cot, 1.0, xi)
                sc.check('vat', f'{rows}x{n} xi={xi}', 'cpu-f32 x_adv', sc.max_rel(xa, ref['x_adv']), 1e-6)
                sc.check('vat', f'{rows}x{n} xi={xi}', 'cpu-f32 gd', sc.max_rel(dr.grad, ref['gd'], ref['gd_terms']), sc.TOL_G)
