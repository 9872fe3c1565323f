"""The HBM-bound kernels of csrc/bn.hip and csrc/elementwise.hip through the C ABI, at every launch regime of tests/stream_cases.py,
against float64 CPU references of the same float32 inputs.  Outputs are NaN-prefilled, strided operands sit in wider buffers whose
padding must come back bit-unchanged, reduction inputs carry outlier rows; every measured error is appended to
stream_kernel_errors.jsonl, next to the parity_errors.jsonl of tests/parity_tol.py."""
import pytest
import torch
import torch.nn.functional as F

import stream_cases as sc

pytestmark = pytest.mark.gpu

NAN = float('nan')
SENTINEL = 1e6                 # padding columns of inputs
PAD_BITS = 0x5EED5EED          # padding columns of outputs (int32 view)


def _lib():
    from reconvat_amd import _lib
    return _lib


def _call(name, *args):
    lib = _lib()
    lib.call(name, *args, lib.stream())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _in(dev, t, ld):
    """[P, C] CPU tensor -> device buffer [P, ld], padding columns = SENTINEL"""
    P, C = t.shape
    buf = torch.full((P, ld), SENTINEL, dtype=torch.float32)
    buf[:, :C] = t
    return buf.to(dev)


def _out(dev, P, C, ld, start=None):
    """device buffer [P, ld]: NaN (or `start`) in the C live columns, PAD_BITS in the padding"""
    buf = torch.empty(P, ld, dtype=torch.float32)
    buf.view(torch.int32).fill_(PAD_BITS)
    buf[:, :C] = NAN if start is None else start
    return buf.to(dev)


def _pad_intact(buf, C):
    pad = buf.view(torch.int32)[:, C:]
    return bool((pad == PAD_BITS).all().item())


def _ws(dev, C):
    """a zeroed BatchNorm workspace (the documented contract of rv_bn_workspace_bytes)"""
    return torch.zeros(_lib().load().rv_bn_workspace_bytes(C) // 8, dtype=torch.float64, device=dev)


def _scatter(dev, a, b):
    """float64 sums [C], [C] -> a workspace [NREP][2][C] whose replicas hold uneven shares (one of them negative) that add up to them"""
    w = torch.tensor([0.31, -0.17, 0.4, 0.06, 0.2, 0.09, 0.08, 0.03], dtype=torch.float64)
    assert w.numel() == sc.RV_BN_NREP
    s = torch.stack([a, b]).double()
    parts = w[:, None, None] * s
    parts[-1] = s - parts[:-1].sum(0)
    return parts.reshape(-1).to(dev)


NBT0 = 5


def bn_fwd(dev, pr, training, slope=sc.SLOPE, res=False, z_ld=None, y_ld=None, res_ld=None, sums=None, z=None, state=None):
    C, P = pr['C'], pr['P']
    z_ld, y_ld, res_ld = z_ld or C, y_ld or C, res_ld or C
    o = {'C': C, 'P': P, 'z_ld': z_ld}
    o['z'] = _in(dev, pr['z'], z_ld) if z is None else z
    z0 = o['z'].clone()
    o['y'] = _out(dev, P, C, y_ld)
    rb = _in(dev, pr['res'], res_ld) if res else None
    o['gamma'], o['beta'] = pr['gamma'].to(dev), pr['beta'].to(dev)
    if state is None:
        state = (pr['rm'].to(dev), pr['rv'].to(dev), torch.full((), NBT0, dtype=torch.long, device=dev))
    o['rm'], o['rv'], o['nbt'] = state
    o['coef'] = torch.full((5 * C,), NAN, device=dev)
    o['ws'] = _ws(dev, C)
    if sums is not None:
        o['ws'].copy_(sums)
    _call('rv_bn_lrelu_fwd', _ptr(o['z']), z_ld, P, C, _ptr(o['gamma']), _ptr(o['beta']), _ptr(o['rm']), _ptr(o['rv']), _ptr(o['nbt']),
          sc.MOMENTUM, sc.EPS, int(training), slope, _ptr(rb), res_ld if res else 0, _ptr(o['y']), y_ld, _ptr(o['coef']), _ptr(o['ws']),
          0 if sums is None else 1)
    torch.cuda.synchronize()
    assert torch.equal(o['z'], z0), 'the forward wrote into its input'
    assert _pad_intact(o['y'], C), 'the forward wrote into the padding of y'
    return o


def check_fwd(where, case, o, ref, training):
    C = o['C']
    body, rows = sc.body_and_rows(o['y'][:, :C], ref['y'])
    sc.check(where, case, 'y', body, sc.TOL, log=True)
    sc.check(where, case, 'y outlier rows', rows, sc.TOL, log=True)
    coef = o['coef'].view(5, C)
    for k, (e, t) in sc.bn_coef_errors(coef, ref, bool(training)).items():
        sc.check(where, case, k, e, t, log=True)
    if training == 1:
        for k, (e, t) in sc.bn_running_errors(o['rm'], o['rv'], ref).items():
            sc.check(where, case, k, e, t, log=True)
    assert int(o['nbt'].item()) == NBT0 + (1 if training == 1 else 0)


def bn_bwd(dev, pr, o, slope=sc.SLOPE, frozen=0, dy_ld=None, dz_ld=None, with_params=True, param_start=None, sums=None):
    """backward of the forward `o` (its z buffer and its coef)"""
    C, P = pr['C'], pr['P']
    dy_ld, dz_ld = dy_ld or C, dz_ld or C
    dy = _in(dev, pr['dy'], dy_ld)
    b = {'dz': _out(dev, P, C, dz_ld), 'ws': _ws(dev, C), 'dgamma': None, 'dbeta': None}
    if with_params:
        b['dgamma'] = torch.full((C,), NAN, device=dev) if param_start is None else param_start[0].to(dev)
        b['dbeta'] = torch.full((C,), NAN, device=dev) if param_start is None else param_start[1].to(dev)
    if sums is not None:
        b['ws'].copy_(sums)
    _call('rv_bn_lrelu_bwd', _ptr(dy), dy_ld, _ptr(o['z']), o['z_ld'], P, C, _ptr(o['coef']), slope, frozen, _ptr(b['dz']), dz_ld,
          _ptr(b['dgamma']), _ptr(b['dbeta']), 0 if param_start is None else 1, _ptr(b['ws']), 0 if sums is None else 1)
    torch.cuda.synchronize()
    assert _pad_intact(b['dz'], C), 'the backward wrote into the padding of dz'
    return b


def check_bwd(where, case, b, ref, C, param_start=None):
    body, rows = sc.body_and_rows(b['dz'][:, :C], ref['dz'], ref['dz_terms'])
    sc.check(where, case, 'dz', body, sc.TOL_G, log=True)
    sc.check(where, case, 'dz outlier rows', rows, sc.TOL_G, log=True)
    if b['dgamma'] is not None:
        s0 = (0.0, 0.0) if param_start is None else (param_start[0].double(), param_start[1].double())
        sc.check(where, case, 'dgamma', sc.max_rel(b['dgamma'].double().cpu() - s0[0], ref['dgamma']), sc.TOL_G, log=True)
        sc.check(where, case, 'dbeta', sc.max_rel(b['dbeta'].double().cpu() - s0[1], ref['dbeta']), sc.TOL_G, log=True)


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(sc.BN_CASES), ids=sc.bn_id)
def test_bn_training_forward_and_backward(dev, case):
    C, P = case
    pr = sc.bn_problem(C, P, True)
    ref = sc.bn_reference(pr, True)
    o = bn_fwd(dev, pr, 1)
    check_fwd('bn training', sc.bn_id(case), o, ref, 1)
    b = bn_bwd(dev, pr, o)
    check_bwd('bn training', sc.bn_id(case), b, ref, C)


@pytest.mark.parametrize('case', list(sc.BN_CASES), ids=sc.bn_id)
def test_bn_eval_forward_and_frozen_backward(dev, case):
    C, P = case
    pr = sc.bn_problem(C, P, False)
    ref = sc.bn_reference(pr, False)
    o = bn_fwd(dev, pr, 0)
    check_fwd('bn eval', sc.bn_id(case), o, ref, 0)
    assert torch.equal(o['rm'].cpu(), pr['rm']) and torch.equal(o['rv'].cpu(), pr['rv'])
    assert not bool(o['ws'].any().item()), 'an eval forward launches no reduction'
    b = bn_bwd(dev, pr, o, frozen=1)
    check_bwd('bn eval', sc.bn_id(case), b, ref, C)
    # frozen with dgamma = NULL: no reduction is launched, the workspace stays zero, dz is the same
    b2 = bn_bwd(dev, pr, o, frozen=1, with_params=False)
    assert not bool(b2['ws'].any().item())
    assert torch.equal(b2['dz'][:, :C], b['dz'][:, :C])


@pytest.mark.parametrize('case', sc.BN_RES_CASES, ids=sc.bn_id)
def test_bn_residual_with_its_own_stride(dev, case):
    C, P = case
    pr = sc.bn_problem(C, P, True)
    ref = sc.bn_reference(pr, True, res=True)
    o = bn_fwd(dev, pr, 1, res=True, res_ld=C + 8)
    check_fwd('bn res_ld', sc.bn_id(case), o, ref, 1)


@pytest.mark.parametrize('case', sc.BN_OPTION_CASES, ids=sc.bn_id)
def test_bn_strided_operands(dev, case):
    """z_ld, y_ld, dy_ld, dz_ld all different, all > C, all multiples of 4"""
    C, P = case
    pr = sc.bn_problem(C, P, True)
    ref = sc.bn_reference(pr, True)
    o = bn_fwd(dev, pr, 1, z_ld=C + 4, y_ld=C + 12)
    check_fwd('bn strided', sc.bn_id(case), o, ref, 1)
    b = bn_bwd(dev, pr, o, dy_ld=C + 8, dz_ld=C + 16)
    check_bwd('bn strided', sc.bn_id(case), b, ref, C)


@pytest.mark.parametrize('case', sc.BN_OPTION_CASES, ids=sc.bn_id)
def test_bn_without_activation(dev, case):
    C, P = case
    pr = sc.bn_problem(C, P, True, slope=1.0)
    ref = sc.bn_reference(pr, True, slope=1.0)
    o = bn_fwd(dev, pr, 1, slope=1.0)
    check_fwd('bn slope=1', sc.bn_id(case), o, ref, 1)
    b = bn_bwd(dev, pr, o, slope=1.0)
    check_bwd('bn slope=1', sc.bn_id(case), b, ref, C)


@pytest.mark.parametrize('case', sc.BN_OPTION_CASES, ids=sc.bn_id)
def test_bn_param_accumulate(dev, case):
    C, P = case
    pr = sc.bn_problem(C, P, True)
    ref = sc.bn_reference(pr, True)
    o = bn_fwd(dev, pr, 1)
    start = (torch.linspace(-300, 500, C), torch.linspace(200, -100, C))
    b = bn_bwd(dev, pr, o, param_start=start)
    check_bwd('bn param_accumulate', sc.bn_id(case), b, ref, C, param_start=start)


@pytest.mark.parametrize('case', sc.BN_OPTION_CASES, ids=sc.bn_id)
def test_bn_sums_ready_folds_every_replica(dev, case):
    """the workspace arrives filled (a conv epilogue's job): float64 host sums, spread unevenly over all the replicas"""
    C, P = case
    pr = sc.bn_problem(C, P, True)
    ref = sc.bn_reference(pr, True)
    z = pr['z'].double()
    o = bn_fwd(dev, pr, 1, sums=_scatter(dev, z.sum(0), (z * z).sum(0)))
    check_fwd('bn sums_ready', sc.bn_id(case), o, ref, 1)
    b = bn_bwd(dev, pr, o, sums=_scatter(dev, ref['dbeta'], ref['dgamma']))
    check_bwd('bn sums_ready', sc.bn_id(case), b, ref, C)


@pytest.mark.parametrize('case', sc.BN_OPTION_CASES, ids=sc.bn_id)
def test_bn_deferred_running_update_is_bit_identical(dev, case):
    """training = 2 leaves the running statistics alone; rv_bn_running_update / rv_bn_running_update_table then give the bits of a
    training = 1 forward (the claim in the comment on bn_momentum_update), for 1 and for 3 queued updates of a layer.  Both forwards
    take the SAME host-computed sums (sums_ready = 1): the order of the reduction's float64 atomics is then not part of the comparison."""
    C, P = case
    pr = sc.bn_problem(C, P, True)
    zc = [pr['z'], pr['z'].flip(0) * 0.75 + 0.5, pr['z'] * 1.25 - 0.25]
    zs = [z.to(dev) for z in zc]
    sums = [_scatter(dev, z.double().sum(0), (z.double() ** 2).sum(0)) for z in zc]

    def fresh():
        return pr['rm'].to(dev), pr['rv'].to(dev), torch.full((), NBT0, dtype=torch.long, device=dev)
    # the fused update, three forwards in sequence on one layer's state
    fused, snap = fresh(), []
    for z, sm in zip(zs, sums):
        o1 = bn_fwd(dev, pr, 1, z=z, state=fused, sums=sm)
        snap.append((fused[0].clone(), fused[1].clone(), int(fused[2].item()), o1))
    # deferred, one by one
    single = fresh()
    coefs = []
    for k, z in enumerate(zs):
        before = [t.clone() for t in single]
        o2 = bn_fwd(dev, pr, 2, z=z, state=single, sums=sums[k])
        assert all(torch.equal(a, b) for a, b in zip(before, single)), 'training = 2 touched the running statistics'
        o1 = snap[k][3]
        assert torch.equal(o2['y'][:, :C], o1['y'][:, :C]) and torch.equal(o2['coef'], o1['coef'])
        _call('rv_bn_running_update', _ptr(single[0]), _ptr(single[1]), _ptr(single[2]), _ptr(o2['coef']), C, sc.MOMENTUM)
        torch.cuda.synchronize()
        assert torch.equal(single[0], snap[k][0]) and torch.equal(single[1], snap[k][1]) and int(single[2].item()) == snap[k][2]
        coefs.append(o2['coef'])
    # the table form: layer 0 with one queued update, layer 1 with three
    la, lb = fresh(), fresh()
    table = torch.tensor([la[0].data_ptr(), la[1].data_ptr(), la[2].data_ptr(), C, 0, 1,
                          lb[0].data_ptr(), lb[1].data_ptr(), lb[2].data_ptr(), C, 1, 3,
                          coefs[0].data_ptr(), coefs[0].data_ptr(), coefs[1].data_ptr(), coefs[2].data_ptr()], dtype=torch.long, device=dev)
    _call('rv_bn_running_update_table', _ptr(table), 2, sc.MOMENTUM)
    torch.cuda.synchronize()
    assert torch.equal(la[0], snap[0][0]) and torch.equal(la[1], snap[0][1]) and int(la[2].item()) == NBT0 + 1
    assert torch.equal(lb[0], snap[2][0]) and torch.equal(lb[1], snap[2][1]) and int(lb[2].item()) == NBT0 + 3


@pytest.mark.parametrize('r', sc.BN_R)
@pytest.mark.parametrize('case', sc.BN_OPTION_CASES, ids=sc.bn_id)
def test_bn_conditioning(dev, case, r):
    """Unit-variance channels at mean r.  The reduction keeps float32 per-thread partials of z^2 (up to 256 pixels) and folds them in
    float64, so var = E[z^2] - mean^2 loses about r^2 float32 ulps.  r = 1 and r = 10 meet the tolerances of every other test.
    r = 100 does NOT and is not asked to; it is measured against what float32 CPU batch_norm makes of the same input, and held
    to R100_FACTOR x that error: a guard on the summation scheme, not a statement that the result is accurate there.
    Measured on the MI355X: see DESIGN.md section 4."""
    C, P = case
    pr = sc.bn_problem(C, P, True, r)
    ref = sc.bn_reference(pr, True)
    o = bn_fwd(dev, pr, 1)
    where, cid = f'bn conditioning r={r}', sc.bn_id(case)
    if r < 100:
        check_fwd(where, cid, o, ref, 1)
        check_bwd(where, cid, bn_bwd(dev, pr, o), ref, C)
        return
    y32 = F.leaky_relu(F.batch_norm(pr['z'].t()[None], None, None, pr['gamma'], pr['beta'], True, sc.MOMENTUM, sc.EPS), sc.SLOPE)[0].t()
    f32, _ = sc.body_and_rows(y32, ref['y'])
    hip, hip_rows = sc.body_and_rows(o['y'][:, :C], ref['y'])
    inv = ((o['coef'].view(5, C)[1].double().cpu() - ref['coef'][1]).abs() / ref['coef'][1]).max().item()
    peak = ref['y'][1:P - 1].abs().max().item()
    for key, val in (('f32 cpu y err / max|y|', f32), ('y outlier rows', hip_rows), ('invstd rel err', inv), ('max abs err of y', hip * peak),
                     ('f32 cpu max abs err of y', f32 * peak), ('ratio hip / f32 cpu', hip / f32)):
        sc.check(where, cid, key, val, float('inf'), log=True)
    print(f'{where} {cid}: invstd rel err {inv:.3g}, max abs err of y {hip * peak:.3g}, float32 CPU {f32 * peak:.3g}, ratio {hip / f32:.3g}')
    sc.check(where, cid, 'y err / max|y|', hip, sc.R100_FACTOR * f32, log=True)


# ---------------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------------
def _dest(dev, N, accumulate):
    """[N + 4]: N live floats (NaN, or a non-zero start when accumulating) and a guard tail"""
    out = torch.full((N + 4,), 7.5)
    start = torch.linspace(3.0, -2.0, N) if accumulate else None
    out[:N] = start if accumulate else NAN
    return out.to(dev), (start.double() if accumulate else 0.0)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('M,N,ld,off,regime', sc.COLSUM_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else v['path'])
def test_colsum(dev, M, N, ld, off, regime, accumulate):
    buf = sc.colsum_input(M, N, ld, off)
    ref = sc.colsum_view(buf, M, N, ld, off).double().sum(0)
    xb = buf.to(dev)
    assert xb.data_ptr() % 16 == 0
    out, start = _dest(dev, N, accumulate)
    _call('rv_colsum', xb.data_ptr() + 4 * off, ld, M, N, _ptr(out), accumulate)
    torch.cuda.synchronize()
    assert torch.equal(xb.cpu(), buf) and bool((out[N:] == 7.5).all().item())
    sc.check('colsum', f'M{M} N{N} ld{ld} off{off} acc{accumulate}', regime['path'], sc.max_rel(out[:N].double().cpu() - start, ref),
             sc.TOL_COLSUM, log=True)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('M,N,regime', sc.COLSUM_ORDERED_CASES, ids=lambda v: str(v) if not isinstance(v, dict) else 'ordered')
def test_colsum_ordered(dev, M, N, regime, accumulate):
    ld = N + 3
    buf = sc.colsum_input(M, N, ld)
    ref = sc.colsum_view(buf, M, N, ld).double().sum(0)
    xb = buf.to(dev)
    nbytes = _lib().load().rv_colsum_ordered_workspace_bytes(M, N)
    assert nbytes == sc.colsum_ordered_blocks(M) * N * 4
    outs = []
    for _ in range(2):
        ws = torch.full((nbytes // 4,), NAN, device=dev)             # "uninitialised"
        out, start = _dest(dev, N, accumulate)
        _call('rv_colsum_ordered', _ptr(xb), ld, M, N, _ptr(out), accumulate, _ptr(ws))
        torch.cuda.synchronize()
        assert bool((out[N:] == 7.5).all().item())
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), 'the ordered column sum is not reproducible'
    sc.check('colsum_ordered', f'M{M} N{N} acc{accumulate}', 'ordered', sc.max_rel(outs[0][:N].double().cpu() - start, ref), sc.TOL_COLSUM, log=True)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('C,c0,n', sc.SUMS_FOLD_CASES)
def test_sums_fold(dev, C, c0, n, accumulate):
    g = sc._gen(C, c0, n, 6)
    sums = torch.randn(sc.RV_BN_NREP, 2, C, generator=g, dtype=torch.float64) * 1000
    ref = sums.sum(0).reshape(-1)[c0:c0 + n]
    out, start = _dest(dev, n, accumulate)
    sg = sums.to(dev)
    _call('rv_sums_fold', _ptr(sg), C, c0, n, _ptr(out), accumulate)
    torch.cuda.synchronize()
    assert bool((out[n:] == 7.5).all().item())
    sc.check('sums_fold', f'C{C} c0{c0} n{n} acc{accumulate}', 'fold', sc.max_rel(out[:n].double().cpu() - start, ref), sc.TOL_COLSUM, log=True)


# ---------------------------------------------------------------------------------------------------------------------
# mean-reduced losses and norms
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', list(sc.REDUCE_CASES))
@pytest.mark.parametrize('kind', list(sc.REDUCE_KINDS))
def test_reduce_mean(dev, kind, n):
    p, t = sc.reduce_input(kind, n, sc.REDUCE_CASES[n][1])
    ref = sc.reduce_reference(kind, p, t)
    pg, tg = p.to(dev), (t.to(dev) if kind in ('bce', 'mse') else None)
    nws = _lib().load().rv_reduce_workspace_bytes(n) // 4
    assert nws == sc.reduce_parts(n)['parts']
    ticket = torch.zeros(1, dtype=torch.int32, device=dev)
    outs = []
    for tk in (None, ticket, ticket):
        out = torch.full((2,), NAN, device=dev)
        ws = torch.full((nws,), NAN, device=dev)
        _call('rv_reduce_mean', sc.REDUCE_KINDS[kind], _ptr(pg), _ptr(tg), n, _ptr(out), _ptr(ws), _ptr(tk))
        torch.cuda.synchronize()
        assert int(ticket.item()) == 0, 'the ticket word is not left zero'
        assert out[1].item() != out[1].item()                        # (the float behind the result is untouched)
        outs.append(out[0].item())
    sc.check('reduce_mean', f'{kind} n={n}', 'rel err', abs(outs[0] - ref.item()) / abs(ref.item()), sc.TOL, log=True)
    assert outs[0] == outs[1] == outs[2], ('two-launch form, ticket form, ticket form again', outs)


# ---------------------------------------------------------------------------------------------------------------------
# grid-stride elementwise kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', sc.GRID_STRIDE_N)
@pytest.mark.parametrize('kind', ['bce', 'mse'])
def test_loss_bwd(dev, kind, n):
    p, t = sc.loss_bwd_input(kind, n)
    ref = sc.loss_bwd_reference(kind, p, t, 1.7)
    gp = torch.full((n + 1,), NAN, device=dev)
    gp[n] = 7.5
    pg, tg, gout = p.to(dev), t.to(dev), torch.tensor([1.7], device=dev)
    _call('rv_loss_bwd', sc.REDUCE_KINDS[kind], _ptr(pg), _ptr(tg), n, _ptr(gout), _ptr(gp))
    torch.cuda.synchronize()
    assert gp[n].item() == 7.5
    got = gp[:n].double().cpu()
    if kind == 'bce':                                                # elements 0, 1: p = 0 and p = 1, torch's clamp of the denominator
        sc.check('loss_bwd', f'bce n={n}', 'clamped', ((got[:2] - ref[:2]).abs() / ref[:2].abs()).max().item(), sc.TOL_G, log=True)
        got, ref = got[2:], ref[2:]
    sc.check('loss_bwd', f'{kind} n={n}', 'body', sc.max_rel(got, ref), sc.TOL_G, log=True)


@pytest.mark.parametrize('n', sc.GRID_STRIDE_N)
def test_clip_scale(dev, n):
    g0 = torch.randn(n, generator=sc._gen(n, 7))
    for norm, max_norm in ((7.3, 3.0), (2.0, 3.0)):
        g = torch.cat([g0, torch.tensor([7.5])]).to(dev)
        total = torch.tensor([norm], device=dev)
        _call('rv_clip_scale', _ptr(g), n, _ptr(total), max_norm)
        torch.cuda.synchronize()
        assert g[n].item() == 7.5
        if norm <= max_norm:
            assert torch.equal(g[:n].cpu(), g0)                      # coefficient clamped at 1
        else:
            ref = g0.double() * (max_norm / (torch.tensor(norm).float().double().item() + 1e-6))
            sc.check('clip_scale', f'n={n}', 'rel err', sc.max_rel(g[:n], ref), sc.TOL_G, log=True)


@pytest.mark.parametrize('n', sc.GRID_STRIDE_N)
def test_adam_step(dev, n):
    """three steps across a StepLR boundary (decay_steps = 2) against the float64 restatement of torch.optim.Adam"""
    gen = sc._gen(n, 8)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (k + 1) for k in range(3)]
    hp = dict(lr0=1e-3, decay_steps=2, decay_rate=0.5, b1=0.9, b2=0.999, eps=1e-8, grad_scale=0.5)
    ref_p, _, _ = sc.adam_reference(p0, grads, **hp)
    abi_p, ref_m, ref_v = sc.adam_reference(p0, grads, abi_floats=True, **hp)
    tail = torch.tensor([7.5])
    p, m, v = (torch.cat([x, tail]).to(dev) for x in (p0, torch.zeros(n), torch.zeros(n)))
    step = torch.zeros((), dtype=torch.long, device=dev)
    for gk in [g.to(dev) for g in grads]:
        _call('rv_adam_step', _ptr(p), _ptr(gk), _ptr(m), _ptr(v), n, _ptr(step), hp['lr0'], hp['decay_steps'], hp['decay_rate'],
              hp['b1'], hp['b2'], hp['eps'], hp['grad_scale'], None)
        _call('rv_counter_add', _ptr(step), 1, None)
    torch.cuda.synchronize()
    assert int(step.item()) == 3 and p[n].item() == m[n].item() == v[n].item() == 7.5
    for key, got, ref in (('p', p, ref_p), ('p (ABI floats)', p, abi_p), ('m', m, ref_m), ('v', v, ref_v)):
        sc.check('adam_step', f'n={n}', key, sc.max_rel(got[:n], ref), sc.TOL_ADAM, log=True)


@pytest.mark.parametrize('which', ['g1', 'g2', 'both'])
@pytest.mark.parametrize('M,N', sc.SIGMOID_BWD_CASES)
def test_sigmoid_bwd(dev, M, N, which):
    gen = sc._gen(M, N, 9)
    g1, g2 = torch.randn(M, N, generator=gen), torch.randn(M, N, generator=gen)
    y = torch.sigmoid(torch.randn(M, N, generator=gen) * 3)
    ld1, ld2, ldy, ldz = N + 1, N + 3, N + 2, N + 5
    use1, use2 = which in ('g1', 'both'), which in ('g2', 'both')
    ref = ((g1.double() if use1 else 0.0) + (g2.double() if use2 else 0.0)) * y.double() * (1 - y.double())
    dz = _out(dev, M, N, ldz)
    b1, b2, by = (_in(dev, g1, ld1) if use1 else None), (_in(dev, g2, ld2) if use2 else None), _in(dev, y, ldy)
    _call('rv_sigmoid_bwd', _ptr(b1), ld1, _ptr(b2), ld2, _ptr(by), ldy, _ptr(dz), ldz, M, N)
    torch.cuda.synchronize()
    assert _pad_intact(dz, N)
    sc.check('sigmoid_bwd', f'M{M} N{N}', which, sc.max_rel(dz[:, :N], ref), sc.TOL_G, log=True)


@pytest.mark.parametrize('xi', sc.VAT_XI)
@pytest.mark.parametrize('n', sc.VAT_N)
@pytest.mark.parametrize('rows', sc.VAT_ROWS)
def test_vat_perturb(dev, rows, n, xi):
    x, d, g = sc.vat_input(rows, n)
    prescale = 3.0
    ref = sc.vat_reference(x, d, g, prescale, xi)
    xg, dg, gg = x.to(dev), d.to(dev), g.to(dev)
    case = f'rows{rows} n{n} xi={xi}'

    def fwd(dd, with_outs):
        o = [torch.cat([torch.full((rows * n,), NAN), torch.tensor([7.5])]).to(dev) for _ in range(3)]
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        _call('rv_vat_perturb_fwd', _ptr(xg), _ptr(dd), rows, n, prescale, xi, _ptr(o[0]), _ptr(o[1]) if with_outs else None,
              _ptr(o[2]) if with_outs else None, _ptr(flag))
        torch.cuda.synchronize()
        assert all(t[rows * n].item() == 7.5 for t in o)
        return [t[:rows * n].view(rows, n) for t in o], int(flag.item())
    (xa, r, dn), flag = fwd(dg, True)
    assert flag == 0
    sc.check('vat_perturb_fwd', case, 'x_adv', sc.max_rel(xa, ref['x_adv']), 1e-6, log=True)
    sc.check('vat_perturb_fwd', case, 'r', sc.max_rel(r, ref['r']), 1e-5, log=True)
    sc.check('vat_perturb_fwd', case, 'dn', sc.max_rel(dn, ref['dn']), 1e-5, log=True)
    (xa2, r2, dn2), flag = fwd(dg, False)
    assert flag == 0 and torch.equal(xa2, xa) and bool(torch.isnan(r2).all().item()) and bool(torch.isnan(dn2).all().item())
    gd = torch.cat([torch.full((rows * n,), NAN), torch.tensor([7.5])]).to(dev)
    _call('rv_vat_perturb_bwd', _ptr(gg), _ptr(xg), _ptr(dg), rows, n, prescale, xi, _ptr(gd))
    torch.cuda.synchronize()
    assert gd[rows * n].item() == 7.5
    sc.check('vat_perturb_bwd', case, 'gd', sc.max_rel(gd[:rows * n].view(rows, n), ref['gd'], ref['gd_terms']), sc.TOL_G, log=True)
    # an all-zero row: 0/0 -> NaN in r -> the flag; the other rows are what they were
    dz = d.clone()
    dz[rows - 1] = 0.0
    (xa3, _, _), flag = fwd(dz.to(dev), True)
    assert flag == 1
    assert torch.equal(xa3[:rows - 1], xa[:rows - 1])
