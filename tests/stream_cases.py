"""Case table, launch arithmetic and float64 references for the HBM-bound kernels of csrc/bn.hip and csrc/elementwise.hip.

The kernels' launch arithmetic (pixels per thread, grid caps, path choices) lives in small host functions of the two .hip
files; it is restated here in Python, and every case below carries the regime it is meant to reach.  tests/test_stream_cases.py
asserts on the CPU that each case lands in its regime, that the float32 CPU reference alone meets the tolerances, and that
a dropped / double-counted outlier row moves a result by >= 10x its tolerance; tests/test_stream_kernels_gpu.py runs the
kernels through the C ABI.  A shape edit can therefore not fall back to the trivial launch silently.

Detection is by construction, not by tight tolerances: the first and last row of every reduction input are +-40 sigma
outliers (distinct per channel, opposite sign), outputs are NaN-prefilled, strided operands sit in wider buffers whose
padding must stay bit-unchanged, accumulating forms start from a non-zero destination.
"""
import json
import os

import torch

import parity_tol

TOL = 2e-5            # forward, relative to max |reference|          (tests/test_ops_gpu.py)
TOL_G = 1e-4          # backward
TOL_COLSUM = 1e-5
TOL_ADAM = 1e-5
TOL_STAT = 1e-5       # batch mean in units of the channel's std, batch variance in units of the variance
TOL_INVSTD = 5e-6     # relative
OUTLIER = 40.0        # in units of the data's standard deviation
KINK_GUARD = 1e-3     # no pre-activation of a BatchNorm case lies closer to the leaky-ReLU kink than this (see bn_problem)
R100_FACTOR = 100.0   # r = 100: kernel error < this x the float32 CPU batch_norm error

EPS, MOMENTUM, SLOPE = 1e-5, 0.1, 0.01

# ---------------------------------------------------------------------------------------------------------------------
# launch arithmetic
# ---------------------------------------------------------------------------------------------------------------------
RV_BN_NREP = 8                 # csrc/common.h
BN_PIX_PER_THREAD = 16         # csrc/bn.hip
BN_MAXBLK = 768                # csrc/bn.hip: bn_apply_blocks (forward and backward cap)


def cdiv(a, b):
    return (a + b - 1) // b


def bn_ppt(P, PL):
    """mirrors bn_ppt() of csrc/bn.hip"""
    ppt = P // (PL * 512)
    ppt = (ppt + 3) & ~3
    return min(max(ppt, BN_PIX_PER_THREAD), 256)


def bn_reduce_launch(P, C):
    """mirrors rv_internal_bn_stats() / rv_internal_bn_bwd_stats() and the thread mapping of bn_reduce_k (csrc/bn.hip)"""
    C4 = C // 4
    PL = 256 // C4
    ppt = bn_ppt(P, PL)
    blocks = cdiv(P, PL * ppt)
    return {'PL': PL, 'idle_threads': 256 - PL * C4, 'ppt': ppt, 'reduce_blocks': blocks, 'replicas': min(blocks, RV_BN_NREP),
            'replica_wrap': blocks > RV_BN_NREP, 'reduce_masked_tail': blocks * PL * ppt > P}


def bn_apply_blocks(total):
    """mirrors bn_apply_blocks() of csrc/bn.hip"""
    b = min(cdiv(total, 256), BN_MAXBLK)
    return cdiv(b, 3) * 3


def bn_apply_launch(P, C, bwd):
    """mirrors the launch of bn_apply_k and its `fixed` test, `pstep` and loop trip counts (csrc/bn.hip)"""
    C4 = C // 4
    total = P * C4
    blocks = bn_apply_blocks(total)
    stride = blocks * 256
    fixed = stride % C4 == 0
    out = {'C4': C4, 'apply_blocks': blocks, 'fixed': fixed}
    if fixed:
        unr = 4 if bwd else 8
        pstep = stride // C4
        out['pstep'] = pstep
        out['trips'] = cdiv(P, unr * pstep)                       # of the thread that starts at pixel 0
        last = (out['trips'] - 1) * unr * pstep                   # ... whose last trip is partly masked when
        out['last_trip_masked'] = last + (unr - 1) * pstep >= P
        out['pixels_per_thread'] = cdiv(P, pstep)
    else:
        out['passes'] = cdiv(total, stride)                       # grid-stride iterations of the generic loop
    return out


def colsum_path(N, ld, M, aligned16=True):
    """mirrors the path choice and `rpt` of rv_colsum() (csrc/elementwise.hip)"""
    if N % 4 == 0 and N <= 256 and ld % 4 == 0 and aligned16 and M >= 1024:
        PL = 256 // (N // 4)
        rpt = min(max(M // (PL * 512), 4), 64)
        return {'path': 'vec', 'PL': PL, 'rpt': rpt, 'blocks': cdiv(M, PL * rpt)}
    return {'path': 'generic', 'col_blocks': cdiv(N, 64), 'row_blocks': cdiv(M, 256), 'row_tail': M % 256 != 0}


def colsum_ordered_blocks(M):
    """mirrors colsum_ordered_blocks() of csrc/elementwise.hip"""
    return min(max(cdiv(M, 256), 1), 1024)


def colsum_ordered_launch(M, N):
    """mirrors rv_colsum_ordered() (csrc/elementwise.hip)"""
    nblk = colsum_ordered_blocks(M)
    return {'nblk': nblk, 'rpb': cdiv(M, nblk), 'fold_blocks': cdiv(N, 256)}


def grid_for(n):
    """mirrors grid_for() of csrc/elementwise.hip"""
    return min(max(cdiv(n, 256), 1), 4096)


def grid_stride_passes(n):
    return cdiv(n, grid_for(n) * 256)


def reduce_parts(n):
    """mirrors rv_reduce_mean(): one partial per 2 048 elements; the fold walks them 256 at a time (csrc/elementwise.hip)"""
    parts = cdiv(n, 2048)
    return {'parts': parts, 'fold_passes': cdiv(parts, 256)}


# ---------------------------------------------------------------------------------------------------------------------
# case tables: shape -> the regime it has to reach (keys of the dicts the functions above return)
# ---------------------------------------------------------------------------------------------------------------------
BN_CASES = {
    # (C, P): (reduce regime, forward apply regime, backward apply regime)
    (128, 70001): ({'PL': 8, 'ppt': 20, 'reduce_blocks': 438, 'replicas': 8, 'reduce_masked_tail': True},
                   {'apply_blocks': 768, 'fixed': True, 'pstep': 6144, 'trips': 2, 'last_trip_masked': True},
                   {'apply_blocks': 768, 'fixed': True, 'trips': 3}),
    (16, 9001): ({'reduce_blocks': 9, 'replica_wrap': True, 'replicas': 8},
                 {'fixed': True, 'pixels_per_thread': 1, 'apply_blocks': 141}, {'fixed': True, 'pixels_per_thread': 1}),
    (20, 1000): ({'PL': 51, 'idle_threads': 1}, {'C4': 5, 'fixed': False, 'passes': 1}, {'fixed': False, 'passes': 1}),
    (20, 40009): ({'PL': 51}, {'fixed': False, 'apply_blocks': 768, 'passes': 2}, {'fixed': False, 'apply_blocks': 768, 'passes': 2}),
    (124, 300): ({'PL': 8, 'idle_threads': 8}, {'C4': 31, 'fixed': False}, {'C4': 31, 'fixed': False}),
    (24, 1349): ({'PL': 42, 'idle_threads': 4, 'reduce_blocks': 3}, {'C4': 6}, {'C4': 6}),
    (4, 257): ({'PL': 256, 'idle_threads': 0}, {'C4': 1}, {'C4': 1}),
    (8, 2): ({'reduce_blocks': 1}, {'C4': 2}, {'C4': 2}),
}
BN_OPTION_CASES = [(16, 9001), (128, 70001)]        # every option below runs on these; (20, 1000) also runs the residual
BN_RES_CASES = BN_OPTION_CASES + [(20, 1000)]
BN_R = [1, 10, 100]                                  # conditioning: unit-variance channels at mean r; 100 is measured, not held to TOL


def bn_id(c):
    return f'C{c[0]}_P{c[1]}'


# rv_colsum: (M, N, ld, offset in floats, expected regime)
COLSUM_CASES = [(1025, N, N + pad, 0, {'path': 'vec', 'rpt': 4}) for N in (4, 24, 88, 256) for pad in (0, 4)] + [
    (10243, 256, 256, 0, {'path': 'vec', 'rpt': 5}),
    (1025, 1, 1, 0, {'path': 'generic'}), (1025, 65, 65, 0, {'path': 'generic', 'col_blocks': 2}),
    (1025, 229, 229, 0, {'path': 'generic', 'col_blocks': 4}),
    (1023, 88, 88, 0, {'path': 'generic'}),
    (257, 88, 88, 0, {'path': 'generic', 'row_blocks': 2, 'row_tail': True}),
    (1025, 229, 231, 0, {'path': 'generic'}),
    (1025, 88, 88, 1, {'path': 'generic'}),
]
COLSUM_ORDERED_CASES = [(1000, 65, {'fold_blocks': 1}), (1000, 257, {'fold_blocks': 2}), (262145, 4, {'nblk': 1024, 'rpb': 257})]
SUMS_FOLD_CASES = [(96, 32, 40), (128, 0, 128)]      # (C, c0, n)

# rv_reduce_mean: n -> (regime, outlier amplitude).  At the largest n the mean of |p| needs a larger outlier for one dropped
# element to clear 10 x TOL; the other kinds are quadratic in it.
REDUCE_CASES = {1: ({'parts': 1}, OUTLIER), 255: ({'parts': 1}, OUTLIER), 2048: ({'parts': 1}, OUTLIER), 2049: ({'parts': 2}, OUTLIER),
                524289: ({'parts': 257, 'fold_passes': 2}, 10 * OUTLIER)}
REDUCE_KINDS = {'bce': 0, 'mse': 1, 'abs': 2, 'l2': 3}
GRID_STRIDE_N = [3, 1048576 + 5]                     # rv_loss_bwd, rv_clip_scale, rv_adam_step: one pass / a second pass
SIGMOID_BWD_CASES = [(37, 88), (11156, 94)]          # (M, N); the second is 1048576 + 88 elements
VAT_ROWS, VAT_N, VAT_XI = [1, 5], [1, 63, 64, 65, 229], [1e-1, 1e-6]


# ---------------------------------------------------------------------------------------------------------------------
# measuring and asserting
# ---------------------------------------------------------------------------------------------------------------------
# next to the loss-term errors of tests/parity_tol.py: the project's one directory for measured figures
_OUT = os.path.join(os.path.dirname(parity_tol._OUT), 'stream_kernel_errors.jsonl')


def max_rel(got, ref, floor=0.0):
    """max |got - ref| / max(max |ref|, floor) in float64 on the CPU; NaN when `got` holds one (and NaN is not < any tolerance).
    floor: the magnitude of the terms that cancel in `ref`, where the reference is (nearly) zero by cancellation."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    if ref.numel() == 0:
        return 0.0
    d = (got - ref).abs()
    if bool(torch.isnan(d).any()):
        return float('nan')
    return (d.max() / ref.abs().max().clamp_min(max(float(floor), 1e-30))).item()


def body_and_rows(got, ref, terms=None):
    """Errors of a [P, ...] tensor: rows 1 .. P-2 relative to THEIR maximum (the outlier rows do not loosen it), rows 0 and P-1
    each relative to its own maximum.  terms (optional, same shape): the summands that cancel in `ref`; their maximum over the same
    rows is the floor of the denominator (dz of a batch of 2 is zero up to eps: dd - mean(dd) - xhat mean(dd xhat) cancels)."""
    P = ref.shape[0]
    fl = (lambda s: terms[s].abs().max().item()) if terms is not None else (lambda s: 0.0)
    body = max_rel(got[1:P - 1], ref[1:P - 1], fl(slice(1, P - 1))) if P > 2 else 0.0
    rows = max(max_rel(got[0], ref[0], fl(0)), max_rel(got[P - 1], ref[P - 1], fl(P - 1)))
    return body, rows


def check(where, case, key, err, tol, log=None):
    """Assert one measured error and (log = True: on the device) append it to stream_kernel_errors.jsonl (see _OUT)."""
    err = float(err)
    if log:
        try:
            os.makedirs(os.path.dirname(_OUT), exist_ok=True)
            with open(_OUT, 'a') as fh:
                fh.write(json.dumps({'where': where, 'case': case, 'key': key, 'err': err, 'tol': tol}) + '\n')
        except OSError:
            pass
    assert err < tol, (where, case, key, err, tol)        # (NaN fails)
    return err


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))
    return g


def outlier_rows(width, amp=OUTLIER):
    """(first, last): +-amp x (1 .. 1.25), distinct per column, opposite sign within a column, alternating over columns"""
    c = torch.arange(width, dtype=torch.float64)
    sign = 1.0 - 2.0 * (c % 2)
    first = sign * amp * (1.0 + 0.25 * c / width)
    last = -sign * amp * (1.0 + 0.25 * (c + 0.5) / width)
    return first, last


def put_outliers(x, center=0.0, amp=OUTLIER):
    """x: [M, N] float64, in place"""
    first, last = outlier_rows(x.shape[1], amp)
    x[0] = center + first
    x[-1] = center + last
    return x


_bn_cache = {}


def bn_problem(C, P, training=True, r=None, slope=SLOPE):
    """float32 CPU inputs of one BatchNorm case.  z: unit-variance channels at mean r (default: distinct means in +-0.5) with the
    two outlier rows; dy likewise around 0.  Elements whose float64 pre-activation gamma*xhat+beta falls within KINK_GUARD of the
    leaky-ReLU kink are moved off it: there the float32 kernel and the float64 reference may legitimately pick different branches of
    a discontinuous derivative, and one such element would cost |dy| in dz / dbeta.  The guard depends on the statistics in use, so
    training and eval inputs differ.  Cached and never modified by the tests."""
    key = (C, P, bool(training), r, slope)
    if key in _bn_cache:
        return _bn_cache[key]
    g = _gen(C, P, 1)
    mean = torch.full((C,), float(r), dtype=torch.float64) if r is not None else torch.linspace(-0.5, 0.5, C, dtype=torch.float64)
    z = torch.randn(P, C, generator=g, dtype=torch.float64) + mean
    put_outliers(z, mean)
    dy = put_outliers(torch.randn(P, C, generator=g, dtype=torch.float64))
    pr = {'C': C, 'P': P, 'r': r,
          'gamma': (0.8 + 0.4 * torch.rand(C, generator=g)).float(), 'beta': (0.1 * torch.randn(C, generator=g)).float(),
          'rm': (mean + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)).float(), 'rv': (0.5 + torch.rand(C, generator=g)).float(),
          'res': torch.randn(P, C, generator=g), 'dy': dy.float(), 'z': z.float()}
    if slope != 1.0 and P > 2:
        for _ in range(2):
            ref = bn_reference(pr, training, slope=slope, backward=False)
            zh = ref['zh']
            near = zh.abs() < 2 * KINK_GUARD
            near[0], near[-1] = False, False
            push = torch.where(zh >= 0, 1.0, -1.0) * 4 * KINK_GUARD / ref['coef'][2]
            pr['z'] = torch.where(near, pr['z'].double() + push, pr['z'].double()).float()
    _bn_cache[key] = pr
    return pr


def bn_reference(pr, training, slope=SLOPE, res=False, frozen=None, backward=True, rm=None, rv=None):
    """float64 BatchNorm2d + leaky ReLU (+ residual) and its backward on [P, C], from the float32 inputs"""
    z, gamma, beta = pr['z'].double(), pr['gamma'].double(), pr['beta'].double()
    rm0, rv0 = (pr['rm'] if rm is None else rm).double(), (pr['rv'] if rv is None else rv).double()
    n = z.shape[0]
    out = {}
    if training:
        mean, var = z.mean(0), z.var(0, unbiased=False)
        unb = var * n / (n - 1) if n > 1 else var
        out['rm'], out['rv'] = (1 - MOMENTUM) * rm0 + MOMENTUM * mean, (1 - MOMENTUM) * rv0 + MOMENTUM * unb
    else:
        mean, var, unb = rm0, rv0, rv0
        out['rm'], out['rv'] = rm0, rv0
    invstd = 1.0 / torch.sqrt(var + EPS)
    scale = gamma * invstd
    shift = beta - mean * scale
    out['coef'] = torch.stack([mean, invstd, scale, shift, unb])
    out['var'] = var
    zh = z * scale + shift
    out['zh'] = zh
    out['y'] = torch.where(zh > 0, zh, zh * slope) + (pr['res'].double() if res else 0.0)
    if backward:
        frozen = (not training) if frozen is None else frozen
        dy = pr['dy'].double()
        dd = torch.where(zh > 0, dy, dy * slope)
        xh = (z - mean) * invstd
        out['dd'] = dd
        out['dz_terms'] = scale * dd
        out['dbeta'], out['dgamma'] = dd.sum(0), (dd * xh).sum(0)
        out['dz'] = scale * (dd if frozen else dd - out['dbeta'] / n - xh * out['dgamma'] / n)
    return out


def bn_coef_errors(got5, ref, training):
    """{name: (error, tolerance)} of a coef block [5, C] (eval: 4 rows) against bn_reference, per the tolerances at the top"""
    got5 = got5.detach().double().cpu()
    mean, invstd, scale, shift, unb = ref['coef']
    std, var = torch.sqrt(ref['var']), ref['var']
    e = {'mean/std': (((got5[0] - mean).abs() / std).max().item(), TOL_STAT),
         'invstd': (((got5[1] - invstd).abs() / invstd).max().item(), TOL_INVSTD),
         'scale': (((got5[2] - scale).abs() / scale.abs()).max().item(), TOL_INVSTD),
         # shift = beta - mean * scale: the two tolerances above, propagated
         'shift': (((got5[3] - shift).abs() / ((TOL_STAT * std + TOL_INVSTD * mean.abs()) * scale.abs() + 1e-7 * shift.abs())).max().item(), 1.0)}
    if training:
        e['unbiased_var/var'] = (((got5[4] - unb).abs() / var).max().item(), TOL_STAT)
    return {k: (float('nan') if v[0] != v[0] else v[0], v[1]) for k, v in e.items()}


def bn_running_errors(rm, rv, ref):
    std, var = torch.sqrt(ref['var']), ref['var']
    return {'running_mean/std': (((rm.double().cpu() - ref['rm']).abs() / std).max().item(), TOL_STAT),
            'running_var/var': (((rv.double().cpu() - ref['rv']).abs() / var).max().item(), TOL_STAT)}


def colsum_input(M, N, ld, off=0):
    """flat float32 buffer of `off` + M x ld floats: data at mean 0.5 with the outlier rows, padding columns = sentinel 1e6"""
    g = _gen(M, N, ld, 2)
    x = put_outliers(torch.randn(M, N, generator=g, dtype=torch.float64) + 0.5, 0.5)
    buf = torch.full((off + M * ld,), 1e6, dtype=torch.float32)
    buf[off:].view(M, ld)[:, :N] = x.float()
    return buf


def colsum_view(buf, M, N, ld, off=0):
    return buf[off:].view(M, ld)[:, :N]


def reduce_input(kind, n, amp):
    """(p, t) float32 for rv_reduce_mean / rv_loss_bwd: BCE probabilities incl. the log-clamp values of test_losses; the last
    element (and the first, for the non-BCE kinds) is the outlier"""
    g = _gen(n, 3)
    if kind == 'bce':
        p = torch.sigmoid(torch.randn(n, generator=g) * 4)
        sp = torch.tensor([0.0, 1.0, 1e-30, 1 - 1e-8])
        t = torch.sigmoid(torch.randn(n, generator=g) * 3)
        if n >= 8:
            p[:4] = sp
        p[n - 1], t[n - 1] = 0.0, amp / OUTLIER                    # a term of 100 t (the clamp) against a typical ~1
        return p, t
    p, t = torch.randn(n, generator=g), torch.randn(n, generator=g)
    p[0] = amp
    p[n - 1] = -amp * 1.125
    return p, t


def reduce_reference(kind, p, t):
    p, t = p.double(), t.double()
    if kind == 'bce':
        # 1 - p is formed in float32 by the kernel and by torch alike; from float32 inputs it is exact or within half an ulp
        lp, lq = torch.log(p).clamp_min(-100), torch.log1p(-p).clamp_min(-100)
        return (-(t * lp + (1 - t) * lq)).mean()
    if kind == 'mse':
        return ((p - t) ** 2).mean()
    if kind == 'abs':
        return p.abs().mean()
    return torch.sqrt((p * p).sum())


def reduce_drop_shift(kind, p, t):
    """relative change of the result when the last element is dropped from the sum (denominator kept)"""
    ref = reduce_reference(kind, p, t)
    n = p.numel()
    if n == 1:
        return 1.0
    if kind == 'l2':
        return abs((torch.sqrt((p[:-1].double() ** 2).sum()) - ref) / ref).item()
    part = reduce_reference(kind, p[:-1], t[:-1]) * (n - 1) / n
    return abs((part - ref) / ref).item()


def loss_bwd_input(kind, n):
    """(p, t) for rv_loss_bwd: BCE probabilities in [1e-3, 1 - 1e-3] with p = 0 and p = 1 (the clamp of the denominator) in front"""
    p, t = reduce_input(kind, max(n, 8), OUTLIER)
    p, t = p[:n].clone(), t[:n].clone()
    if kind == 'bce':
        p = p.clamp(1e-3, 1 - 1e-3)
        p[0], p[1] = 0.0, 1.0
    return p, t


def loss_bwd_reference(kind, p, t, gout):
    """float64 gradient of the mean-reduced loss times gout; BCE with torch's clamp of (1 - p) p at 1e-12"""
    p, t = p.double(), t.double()
    if kind == 'bce':
        return (p - t) / ((1 - p) * p).clamp_min(1e-12) * gout / p.numel()
    return 2 * (p - t) * gout / p.numel()


def adam_reference(p, grads, lr0, decay_steps, decay_rate, b1, b2, eps, grad_scale, abi_floats=False):
    """float64 restatement of torch.optim.Adam (defaults) under StepLR, one step per gradient in `grads`.
    abi_floats: the hyper-parameters as the float32 values that cross the C ABI.  It matters for v only: 1 - float32(0.999) is
    1.3e-5 (relative) away from 0.001, so the kernel's second moment is that far from torch's, and p (through sqrt(v), in an update
    of ~lr) far less.  p is held to torch's own hyper-parameters, m and v to the values the kernel is given."""
    if abi_floats:
        lr0, decay_rate, b1, b2, eps, grad_scale = (torch.tensor(x, dtype=torch.float32).double().item() for x in (lr0, decay_rate, b1, b2, eps, grad_scale))
    p = p.double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, g in enumerate(grads):
        g = g.double() * grad_scale
        lr = lr0 * decay_rate ** (step // decay_steps)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** (step + 1), 1 - b2 ** (step + 1)
        p = p - lr / bc1 * m / (torch.sqrt(v) / bc2 ** 0.5 + eps)
    return p, m, v


def vat_input(rows, n):
    """x in [0.05, 0.95] with clamped elements at both ends, d, g (float32).  Elements 1 and 2 of a row lie OUTSIDE [0, 1] (the clamp
    is active whatever the perturbation), element 0 is exactly 0 (the sign of the perturbation decides, and 0 + r is exact in
    float32), element 3 is exactly 1 -- see vat_reference for the one place where float32 rounding decides."""
    g = _gen(rows, n, 4)
    x = 0.05 + 0.9 * torch.rand(rows, n, generator=g)
    for i, v in enumerate((0.0, -0.25, 1.25, 1.0)):
        if i < n:
            x[:, i] = v
    return x, torch.randn(rows, n, generator=g), torch.randn(rows, n, generator=g)


def vat_reference(x, d, g, prescale, scale):
    """float64 from the float32 inputs.  The clamp mask of the backward is taken on the float32-rounded sum x + r, as the kernel
    and torch's clamp backward both do: at x = 1 and |r| < 6e-8 (xi = 1e-6) the sum rounds back onto the bound."""
    x, d, g = x.double(), d.double() * prescale, g.double()
    nrm = d.norm(dim=-1, keepdim=True)
    dn = d / nrm
    r = scale * dn
    xa = x + r
    inside = (xa.float() >= 0) & (xa.float() <= 1)
    gr = torch.where(inside, g * scale, torch.zeros_like(g))
    gd = (gr - dn * (dn * gr).sum(-1, keepdim=True)) / nrm * prescale
    # gd_terms: gr - dn <dn, gr> cancels to zero for n = 1
    return {'x_adv': xa.clamp(0, 1), 'r': r, 'dn': dn, 'gd': gd, 'gd_terms': (gr.abs() / nrm * prescale).max().item()}
