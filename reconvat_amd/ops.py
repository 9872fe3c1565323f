"""Host-side operators: thin ``torch.autograd.Function`` wrappers over the C ABI of
libreconvat_hip.so.  PyTorch is used for device memory, streams and the autograd tape only; every
numeric kernel is a hand-written HIP kernel (reconvat_amd/csrc).  There is no CPU fallback.

Internal activation layout is NHWC ([B, H=time, W=bins, C]); a tensor handed to a conv may be a channel
slice (view) of a wider buffer -- the pixel stride is taken from ``stride(2)``.
"""
import ctypes
import os
from collections import namedtuple

import torch
from torch.autograd import Function

from . import _lib, plans, tuning
from ._lib import call, invoke, ptr, stream, need_gpu
# kernel selection lives in tuning.py; tools and tests reach its tables and state through these names (the same objects)
from .tuning import ALGO_BF16, WINOGRAD_FAMILIES, _algo_cache, _tune_us, _tune_top, _wgrad_tuned, _wgrad_plans, _wgrad_owner, _gemm_splitk  # noqa: F401

SLOPE = 0.01            # F.leaky_relu default (model/UNet_onset.py:197-198)
BN_MOMENTUM = 0.1       # model/UNet_onset.py:183
BN_EPS = 1e-5

_EPOCH = [0]
# RV_DETERMINISTIC=1 (or ops.DETERMINISTIC[0] = True): bit-reproducible PARAMETER GRADIENTS.  The data path -- forward passes and
# input-gradient chains, hence every loss term and running statistic -- is free of fp32 atomics in every mode; what is order-dependent by
# default are the folds onto the gradient bucket: the table-driven weight-gradient reductions (several passes of a step target the same
# layer: fp32 atomics), the atomic split-K of the parameter-gradient GEMMs with the bias row sums riding on them, the column-sum bias
# gradients.  In this mode the weight-gradient reductions run per layer in stream order (fixed tree, read-modify-write), the
# parameter-gradient GEMMs use the in-order (park + fold) split-K of the data path, column sums the two-pass ordered form.  Slower (see
# `deterministic_ms_per_step` in bench.py's line); the default stays the atomic folds.
DETERMINISTIC = [os.environ.get('RV_DETERMINISTIC') == '1']
_DIRECT = [False]


class ZeroArena:
    """Bump allocator over ONE device buffer that is cleared once per training step: reduction kernels that need
    zero-initialised scratch (BatchNorm sums) take slices instead of issuing a memset per call.  Armed by
    TrainStep (also under hipGraph capture: the clear is the first node and the slice order is deterministic);
    unarmed, `take` falls back to torch.zeros."""

    def __init__(self):
        self.buf = None
        self.off = 0
        self.armed = False

    def begin_step(self, device, nbytes=8 << 20):
        if self.buf is None or self.buf.device != device or self.buf.numel() * 8 < nbytes:
            self.buf = torch.zeros(nbytes // 8, device=device, dtype=torch.float64)
        else:
            self.buf.zero_()
        self.off = 0
        self.armed = True

    def end_step(self):
        self.armed = False

    def take(self, n_doubles, device):
        if self.armed and self.buf.device == device and self.off + n_doubles <= self.buf.numel():
            out = self.buf[self.off:self.off + n_doubles]
            self.off += (n_doubles + 1) & ~1
            return out
        return torch.zeros(n_doubles, device=device, dtype=torch.float64)


ARENA = ZeroArena()


def bn_ws_doubles(c):
    """fp64 elements of one BatchNorm reduction workspace (rv_bn_workspace_bytes: replicated [2C] sums)."""
    return _lib.load().rv_bn_workspace_bytes(c) // 8

_BN_DEFER = [None]

# Two-stream VAT (read by model._Base._step_plan, which then runs _vat_two_streams, and by onset_frames' run_on_batch).  Off by default: TrainStep switches it on once the weights are packed
# by the one-launch plan and the conv autotuner has run (neither tolerates a concurrent second stream).
DUAL_STREAM = [False]
_SIDE = {}


def side_stream(device, idx=0):
    """The idx-th side stream of `device` (created on first use; idx 0 is the U-Net schedule's, the Onsets&Frames
    schedule also uses idx 1)."""
    key = (device.type, device.index, idx)
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


class deferred_bn_updates:
    """Inside this context train-mode BatchNorm forwards use batch statistics but do NOT touch running_mean /
    running_var / num_batches_tracked; the skipped updates are collected and can be replayed (any number of
    times, at the point of the reference's update sequence where they belong) with ``apply()``."""

    def __enter__(self):
        self.prev = _BN_DEFER[0]
        self.items = []
        _BN_DEFER[0] = self.items
        return self

    def __exit__(self, *exc):
        _BN_DEFER[0] = self.prev

    def apply(self):
        for rm, rv, nbt, coef, c in self.items:
            call('rv_bn_running_update', ptr(rm), ptr(rv), ptr(nbt), ptr(coef), c, BN_MOMENTUM, stream())


_REPLAY_KEEP = []          # pinned host tables of captured replays must outlive their hipGraph (captures outside any keep_scope)
_REPLAY_POOL = []          # pre-allocated pinned staging buffers for capture

# Objects a hipGraph capture pins (host tables a captured copy node re-reads at every replay, their device copies) must live exactly
# as long as the graph.  A capture runs inside `keep_scope(owner_list)`: everything pinned during it lands in the OWNER's list
# (TrainStep._keep), which is dropped together with the graph -- so a process may capture and drop any number of steps without
# growing.  Outside a scope the module-level lists above keep the objects for the life of the process (one-off captures in tests).
_KEEP_SCOPE = [None]


class keep_scope:
    def __init__(self, owner_list):
        self.owner = owner_list

    def __enter__(self):
        self.prev = _KEEP_SCOPE[0]
        _KEEP_SCOPE[0] = self.owner
        return self.owner

    def __exit__(self, *exc):
        _KEEP_SCOPE[0] = self.prev


def _keep(obj, fallback):
    (_KEEP_SCOPE[0] if _KEEP_SCOPE[0] is not None else fallback).append(obj)


def _fill_pool(pool, n, numel, dtype=torch.uint8):
    while len(pool) < n:
        pool.append(torch.empty(numel, dtype=dtype).pin_memory())


class _HostTable:
    """Host side of "fill a table, copy it to the device, run one launch".  No host allocation may happen under hipGraph capture and a captured copy node
    re-reads its buffer at every replay: a capture takes a pre-pinned buffer from `pool` (prepare_*) that is never recycled and lives, like the device copy,
    as long as the graph (keep_scope, else `fallback`).  Outside capture: pageable memory, pinned at upload (the pinned allocator is stream-aware)."""

    def __init__(self, what, entry, capacity, pool, fallback, torch_stream, dtype=torch.uint8):
        self.what, self.entry, self.fallback, self.stream, self.n = what, entry, fallback, torch_stream, 0
        self.pinned = torch.cuda.is_current_stream_capturing()
        if self.pinned:
            if not pool:
                raise RuntimeError(f'{what}: no pinned table left for hipGraph capture')
            self.host = pool.pop()
            _keep(self.host, fallback)
        else:
            self.host = torch.empty(capacity * entry, dtype=dtype)
        self.capacity = self.host.numel() // entry

    def slot(self):
        """Host address of the next entry (the caller fills it, then counts it in `n`)."""
        if self.n >= self.capacity:
            raise RuntimeError(f'{self.what}: table full')
        return self.host.data_ptr() + self.n * self.entry * self.host.element_size()

    def upload(self):
        """Device copy of the n filled entries, enqueued on the table's stream (which must be the current one); the table is empty afterwards."""
        used = self.host[:self.n * self.entry]
        table = (used if self.pinned else used.pin_memory()).to(self.stream.device, non_blocking=True)
        table.record_stream(self.stream)
        if self.pinned:
            _keep(table, self.fallback)        # captured: keep the device copy's memory out of the graph pool's reuse
        self.n = 0
        return table


def prepare_replay_pool(n=4):
    """Pinned staging buffers for replay_bn_updates under hipGraph capture (call outside capture)."""
    _fill_pool(_REPLAY_POOL, n, 4096, torch.int64)


def replay_bn_updates(pendings, device):
    """Apply the deferred BatchNorm updates of several passes -- `pendings`: deferred_bn_updates objects in the order of
    the reference's update sequence (an object may appear twice) -- with ONE launch: per layer the updates are chained
    in that order inside the kernel (rv_bn_running_update_table)."""
    layers, order = {}, []
    for pend in pendings:
        for rm, rv, nbt, coef, c in pend.items:
            key = ptr(rm)
            if key not in layers:
                layers[key] = [ptr(rm), ptr(rv), ptr(nbt) or 0, c, []]
                order.append(key)
            layers[key][4].append(ptr(coef))
    if not order:
        return
    head, coefs = [], []
    for key in order:
        rm, rv, nbt, c, lst = layers[key]
        head += [rm, rv, nbt, c, len(coefs), len(lst)]
        coefs += lst
    words = head + coefs
    if not torch.cuda.is_current_stream_capturing():
        prepare_replay_pool()
    tab = _HostTable('replay_bn_updates', 1, len(words), _REPLAY_POOL, _REPLAY_KEEP, torch.cuda.current_stream(device), torch.int64)
    assert len(words) <= tab.capacity, 'BatchNorm replay table larger than the staging buffer'
    tab.host[:len(words)] = torch.tensor(words, dtype=torch.int64)
    tab.n = len(words)
    call('rv_bn_running_update_table', ptr(tab.upload()), len(order), BN_MOMENTUM, stream())


class direct_param_grads:
    """Context manager: while active, conv / BatchNorm backward kernels ACCUMULATE their parameter gradients
    straight into the pre-allocated ``param.grad`` buffers (FlatAdam's flat gradient bucket) and hand autograd
    ``None`` for them -- this removes one add kernel per parameter per graph.  Only for loops that consume
    ``param.grad`` (TrainStep); ``torch.autograd.grad(..., params)`` would not see these gradients."""

    def __enter__(self):
        self.prev = _DIRECT[0]
        _DIRECT[0] = True

    def __exit__(self, *exc):
        _DIRECT[0] = self.prev


# (flat gradient bucket, {side stream: its twin}): backward kernels that run on a side stream accumulate into that stream's
# twin, so concurrent backward chains never read-modify-write the same addresses; FlatAdam.merge_side_grads() adds them in.
SIDE_GRADS = [None]


def _grad_buf(t):
    if not (_DIRECT[0] and t is not None and t.is_leaf and t.requires_grad and t.grad is not None):
        return None
    sg = SIDE_GRADS[0]
    if sg is not None and DUAL_STREAM[0]:
        main, twins = sg                      # twins: {side stream handle: that stream's twin of the flat bucket}
        twin = twins.get(torch.cuda.current_stream(t.device).cuda_stream)
        if twin is not None:
            off = (t.grad.data_ptr() - main.data_ptr()) // 4
            return twin[off:off + t.grad.numel()].view_as(t.grad)
    return t.grad


def drop_packs_of(flat):
    """Forget every packed copy whose source weight lives in the storage of `flat` (FlatAdam's parameter buffer): the cache holds its
    source tensors, so the packs of a model that is gone would otherwise keep its whole parameter buffer alive."""
    sp = flat.untyped_storage().data_ptr()
    for k in [k for k, v in _pack_cache.items() if v[2].untyped_storage().data_ptr() == sp]:
        del _pack_cache[k]


def drop_packs_of_params(params):
    """Forget every packed copy whose source weight shares storage with one of `params` (a model that is going away: _Base.__del__).
    Together with drop_packs_of (FlatAdam.__del__) this is what bounds the cache: entries die with their OWNER, not with their age --
    a live but idle model (an evaluation copy, the frame model while the onset model trains) keeps its packs."""
    sps = set()
    for p in params:
        try:
            sps.add(p.untyped_storage().data_ptr())
        except Exception:  # noqa: BLE001 -- a parameter without storage (meta / already freed)
            pass
    for k in [k for k, v in _pack_cache.items() if v[2].untyped_storage().data_ptr() in sps]:
        del _pack_cache[k]


def invalidate_weight_cache():
    """Call after any out-of-band parameter update (custom optimiser step, load_state_dict)."""
    _EPOCH[0] += 1


# --------------------------------------------------------------------------------------------
# geometry helpers
# --------------------------------------------------------------------------------------------
def _geom(t):
    b, h, w, c = t.shape
    if t.is_contiguous():
        return b, h, w, c, c
    ld = t.stride(2)
    ok = (c == 1 or t.stride(3) == 1) and (h == 1 or t.stride(1) == w * ld) and (b == 1 or t.stride(0) == h * w * ld)
    if not ok or w == 1:
        raise RuntimeError(f'expected an NHWC tensor or a channel slice of one, got shape {tuple(t.shape)} '
                           f'strides {t.stride()}')
    return b, h, w, c, ld


def _new(b, h, w, c, like):
    return torch.empty((b, h, w, c), device=like.device, dtype=torch.float32)


# --------------------------------------------------------------------------------------------
# convolution kinds: how forward / input-gradient / weight-gradient map onto the C ABI
# --------------------------------------------------------------------------------------------
#   kind   PyTorch module                         weight layout
#   c3     Conv2d(k=3, p=1)                       [Cout, Cin, 3, 3]
#   t3     ConvTranspose2d(k=3, p=1)              [Cin, Cout, 3, 3]
#   c1     Conv2d(k=1)                            [Cout, Cin, 1, 1]
#   down   Conv2d(k=2, s=2)                       [Cout, Cin, 2, 2]
#   up     ConvTranspose2d(k=2, s=2, output_size) [Cin, Cout, 2, 2]
def _channels(kind, w):
    if kind in ('t3', 'up'):
        return w.shape[0], w.shape[1]
    return w.shape[1], w.shape[0]


_pack_cache = {}
# Entries die with their OWNER (drop_packs_of / drop_packs_of_params).  Weights packed through the functional API or by modules that
# are not _Base models have no owner: a bounded LRU is the fallback for those (re-inserting a key moves it to the young end; a live
# model's entries are re-inserted by PackPlan.run() every step and by every lazy repack, so they are never the old end for long).
_PACK_CACHE_MAX = int(os.environ.get('RV_PACK_CACHE_MAX', '2048'))


def _pack_put(key, val):
    _pack_cache.pop(key, None)
    _pack_cache[key] = val
    while len(_pack_cache) > _PACK_CACHE_MAX:
        del _pack_cache[next(iter(_pack_cache))]


def _cached(key, w, make):
    """The packed copy of the weight (view) `w` under `key`, repacked when the weight changed: make() -> (packed tensor, rv_pack_weights arguments)."""
    tag = (_EPOCH[0], w._version, tuple(w.shape))
    hit = _pack_cache.get(key)
    if hit is None or hit[0] != tag:
        out, args = make()
        hit = (tag, out, w, args)
        _pack_put(key, hit)
    return hit[1]


def _pack(kind, w, which):
    """Packed weight fragments for `which` in {'fwd', 'dgrad'} (cached per weight version)."""
    return _cached((w.data_ptr(), kind, which), w, lambda: _pack_make(kind, w, which))


def _pack_make(kind, w, which):
    cin, cout = _channels(kind, w)
    scatter = 0
    if kind == 'c3':
        args = (9, cin, cout, 9, cin * 9, 0) if which == 'fwd' else (9, cout, cin, cin * 9, 9, 1)
    elif kind == 't3':
        args = (9, cin, cout, cout * 9, 9, 1) if which == 'fwd' else (9, cout, cin, 9, cout * 9, 0)
    elif kind == 'c1':
        args = (1, cin, cout, 1, cin, 0) if which == 'fwd' else (1, cout, cin, cin, 1, 0)
    elif kind == 'down':
        if which == 'fwd':
            args = (4, cin, cout, 4, cin * 4, 0)
        else:
            args, scatter = (1, cout, 4 * cin, cin * 4, 4, 0), cin
    elif kind == 'up':
        if which == 'fwd':
            args, scatter = (1, cin, 4 * cout, cout * 4, 4, 0), cout
        else:
            args = (4, cout, cin, 4, cout * 4, 0)
    else:
        raise ValueError(kind)
    taps, kdim, ndim, s_k, s_n, flip = args
    plain = 1 if (kdim % 8 != 0 or (ndim <= 2 and not scatter)) else 0
    lib = _lib.load()
    n = lib.rv_packed_weight_floats(taps, kdim, ndim)
    out = torch.empty(n, device=w.device, dtype=torch.float32)
    call('rv_pack_weights', ptr(w), ptr(out), taps, kdim, ndim, s_k, s_n, flip, scatter, plain, stream())
    return out, (taps, kdim, ndim, s_k, s_n, flip, scatter, plain)


def _pack_plain(w, tag, args, numel):
    """Plain [tap][k][n] re-indexed copy of a weight (view) through the packed-weight cache, keyed (pointer, *tag) (part of the PackPlan table)."""
    def make():
        out = torch.empty(numel, device=w.device, dtype=torch.float32)
        call('rv_pack_weights', ptr(w), ptr(out), *args, stream())
        return out, args
    return _cached((w.data_ptr(),) + tag, w, make)


def _pack_rel(rel, f):
    """rel^T [31, F] for the attention kernels (cached per weight version; part of the PackPlan table)."""
    return _pack_plain(rel, ('rel', 'T'), (1, 31, f, 1, 31, 0, 0, 1), 31 * f)            # out[w*F + c] = rel[c*31 + w]


def _lin_t(w2d):
    """Contiguous transposed copy [K, N] of a row-major linear weight view w2d [N, K] (cached per weight version; part of
    the PackPlan table).  The input-gradient GEMM dY @ W then reads BOTH operands along their contiguous dimension
    (rv_gemm's LDS-DMA kernel) instead of gathering W column-wise."""
    n, k = w2d.shape
    assert w2d.stride(1) == 1 and w2d.stride(0) == k
    return _pack_plain(w2d, ('lin', 'T', n, k), (1, k, n, 1, k, 0, 0, 1), k * n).view(k, n)            # out[kk*n + nn] = w[kk + nn*k]


class PackPlan:
    """Every packed weight currently in the cache, repacked by ONE kernel launch (rv_pack_table_run).  Build it after
    a warm-up step has populated the cache, call ``run()`` right after each optimiser step: the cache entries are
    re-tagged as fresh, so the ~100 lazy per-layer pack launches of the next step disappear.  Entries created later
    stay on the lazy path."""

    def __init__(self, device):
        import ctypes
        lib = _lib.load()
        # (the cache is pruned by OWNER -- FlatAdam.__del__ -> drop_packs_of, _Base.__del__ -> drop_packs_of_params --, never by age)
        self.entries = [(k, v) for k, v in _pack_cache.items() if v[2].device == device]
        self.count = len(self.entries)
        if not self.count:
            return
        nbytes = lib.rv_pack_table_entry_bytes() * self.count
        host = (ctypes.c_char * nbytes)()
        total = 0
        for i, (_, (_, out, w, a)) in enumerate(self.entries):
            total = lib.rv_pack_table_fill(host, i, ptr(w), ptr(out), *a)
            if total < 0:
                raise RuntimeError('rv_pack_table_fill: ' + _lib.last_error())
        self.total_blocks = total
        self.table = torch.frombuffer(host, dtype=torch.uint8).clone().to(device)

    def run(self):
        if not self.count:
            return
        call('rv_pack_table_run', ptr(self.table), self.count, self.total_blocks, stream())
        for key, (_, out, w, a) in self.entries:
            _pack_put(key, ((_EPOCH[0], w._version, tuple(w.shape)), out, w, a))


_FWD_MODE = {'c3': 0, 't3': 0, 'c1': 1, 'down': 2, 'up': 3}
_DGRAD_MODE = {'c3': 0, 't3': 0, 'c1': 1, 'down': 3, 'up': 2}


# 'table' (default): the shipped plan table; True: on-line tuning; False: library default tiles (plans.py).  Read at call time and handed to tuning.py.
AUTOTUNE = plans.default_mode()


# BASELINE config 3 as an OPT-IN experiment (default off; the shipped / headline configuration is fp32 end to end): bf16 operands on
# the matrix pipe (fp32 accumulation, statistics, losses, master weights) for the convolutions of the FINAL graphs -- the convs
# whose weights are live; the no_grad target pass and the detached XI*d pass of the power iteration always stay fp32 (at XI = 1e-6
# the perturbation is below one bf16 ulp).  'fwd': forward convs, 'bwd': input- and weight-gradient convs.  Measured
# (tools/bf16_emulation.py): 'fwd' breaks the 1e-3 forward parity bar (frame2 moves by 18 %), 'bwd' leaves every
# loss term and posteriorgram bit-identical and moves the gradients by 0.6 % -- so only 'bwd' is meant to be used.
BF16 = {'fwd': False, 'bwd': False}


class bf16_final_graphs:
    def __init__(self, fwd=False, bwd=True):
        self.want = {'fwd': bool(fwd), 'bwd': bool(bwd)}

    def __enter__(self):
        self.prev = dict(BF16)
        BF16.update(self.want)
        return self

    def __exit__(self, *exc):
        BF16.update(self.prev)


def _conv_call(mode, x, ild, bb, h, wd, cin, out, old, ho, wo, cout, wpack, bias, stats=None, bnbwd=None, accumulate=False, bf16=False):
    """rv_conv_fwd with the per-shape tile choice of tuning.choose_conv (plan table; ops.AUTOTUNE = True: the first eager call of a shape times every
    candidate tile and caches the winner; under hipGraph capture an untuned shape uses the library default).  ``stats`` (fp64 [2*cout], zeroed): the
    conv also leaves the BatchNorm batch statistics of its output there (fused epilogue of the persistent kernel, else a statistics pass -- the tuner
    times whichever the candidate implies).  ``bnbwd`` = (z, coef, slope): the call is an input gradient and ``stats`` receives the backward
    reduction of the BatchNorm whose output gradient is being produced."""
    args = (mode, ptr(x), ild, bb, h, wd, cin, ptr(out), old, ho, wo, cout, ptr(wpack), ptr(bias), 1 if accumulate else 0)
    if bnbwd is not None:
        bz, bcoef, bslope = bnbwd
        tail = (ptr(bz), _geom(bz)[4], ptr(bcoef), float(bslope))
    else:
        tail = (None, 0, None, 0.0)
    force = os.environ.get('RV_FORCE_ALGO') and (mode == 0 or os.environ.get('RV_FORCE_ALGO_ALL'))   # kernel experiments

    def online(key):
        if torch.cuda.is_current_stream_capturing():
            return None
        st = torch.cuda.current_stream()
        lib = _lib.load()
        scratch = ptr(torch.zeros_like(stats)) if stats is not None else None
        targs = args
        if accumulate:          # the timing runs must not touch the buffer that is being accumulated into
            tmp_out = torch.empty(bb * ho * wo * old, device=out.device, dtype=torch.float32)
            targs = args[:7] + (ptr(tmp_out),) + args[8:14] + (0,)
        fams = os.environ.get('RV_TUNE_FAMILIES')
        cands = tuning.conv_candidates(mode, h, wd, cin, cout, winograd=os.environ.get('RV_TUNE_WINOGRAD', '1') != '0',
                                       wino2=os.environ.get('RV_TUNE_WINO2', '1') != '0',
                                       families={int(f, 0) for f in fams.split(',')} if fams else None)

        def run(cand):
            return lib.rv_conv_fwd(*targs, cand | (ALGO_BF16 if bf16 else 0), scratch, *tail, st.cuda_stream)
        return tuning.tune('conv', key, cands, run, lambda cand: tuning.best_of_bursts(lambda: run(cand), st),
                           describe=lambda algo: f'mode={mode} {cin}->{cout} {h}x{wd} B={bb}: algo={algo:#x}')

    algo = tuning.choose_conv(AUTOTUNE, (mode, bb, h, wd, cin, cout, ild, old, stats is not None, bnbwd is not None), bf16,
                              int(os.environ['RV_FORCE_ALGO'], 0) if force else None, online,
                              lambda algo: invoke('rv_conv_fwd', *args, algo, ptr(stats), *tail, stream()))
    if algo is not None:
        call('rv_conv_fwd', *args, algo, ptr(stats), *tail, stream())


def conv_forward_into(kind, x, w, b, out, stats=None, bf16=False):
    """out (NHWC view) = conv(x) ; shapes are taken from the views.  stats: see _conv_call."""
    need_gpu(x, w, out)
    bb, h, wd, cin, ild = _geom(x)
    _, ho, wo, cout, old = _geom(out)
    _conv_call(_FWD_MODE[kind], x, ild, bb, h, wd, cin, out, old, ho, wo, cout, _pack(kind, w, 'fwd'), b, stats, bf16=bf16)


def conv_dgrad_into(kind, dy, w, dx, bn_link=None, accumulate=False, bf16=False, sum_ws=None):
    """dx (NHWC view) (+)= input gradient of the conv given dy (NHWC view).  bn_link: the BnLink of the BatchNorm that
    produced the conv's input -- its backward reduction is then computed in this kernel's epilogue."""
    assert not (accumulate and bn_link is not None)
    bb, h, wd, c, ild = _geom(dy)
    _, ho, wo, co, old = _geom(dx)
    stats = bnbwd = None
    if bn_link is not None and bn_link.usable(dx):
        stats, bnbwd = bn_link.ws, (bn_link.z, bn_link.coef, bn_link.slope)
    elif sum_ws is not None:
        stats = sum_ws                           # plain per-channel sums of dx (ColsumLink): the fused statistics epilogue
    _conv_call(_DGRAD_MODE[kind], dy, ild, bb, h, wd, c, dx, old, ho, wo, co, _pack(kind, w, 'dgrad'), None, stats, bnbwd, accumulate,
               bf16=bf16)
    if bnbwd is not None:
        bn_link.ready = True


class GradShare:
    """One activation consumed by several convs (a block's conv1 + skip, the decoder's skip conv): the first
    input-gradient kernel to run writes the shared buffer and hands it to autograd, the others ACCUMULATE into it
    (rv_conv_fwd accumulate=1) and hand autograd nothing -- no add kernel, no extra pass over the tensor.  Create one per
    forward call and pass it to every consumer; all consumers must run on the same stream."""

    def __init__(self):
        self.buf = None

    def dgrad(self, kind, dy, w, shape, bf16=False):
        if self.buf is None:
            self.buf = torch.empty(shape, device=dy.device, dtype=torch.float32)
            conv_dgrad_into(kind, dy, w, self.buf, bf16=bf16)
            return self.buf
        conv_dgrad_into(kind, dy, w, self.buf, accumulate=True, bf16=bf16)
        return None


class ColsumLink:
    """Connects the conv whose INPUT gradient is dY of a 2x2 up-conv (d_block: conv2d consumes the up-conv's output) with that
    up-conv: the column sums of dY -- the up-conv's bias gradient -- are the per-channel sums of what the producer's input-gradient
    kernel stores, which its fused statistics epilogue provides for free (instead of a colsum pass re-reading dY: 20 launches of
    ~17 us per step)."""

    def __init__(self):
        self.sums = None         # fp64 statistics workspace filled by the producer's dgrad
        self.c = 0               # its channel count


class BnLink:
    """Connects a BatchNorm+activation node with the ONE conv that consumes its output, so that the conv's
    input-gradient kernel can produce the BatchNorm's backward reduction in its epilogue (the gradient of the
    BatchNorm output is exactly that conv's dgrad result -- valid only for a single consumer)."""

    def __init__(self):
        self.z = self.coef = self.ws = None
        self.slope = 0.0
        self.ready = False

    def usable(self, dx):
        return self.ws is not None and self.z is not None and tuple(self.z.shape) == tuple(dx.shape)


class WgradProblem(namedtuple('WgradProblem', 'mode taps u uld hu wu ca v vld hv wv cb bb s_a s_b flip')):
    """The pixel-reduction GEMM behind a conv layer's weight gradient (built by _wgrad_geom): G[tap][a][b] = sum_p U[p + tap][a] * V[p][b] over the pixels of
    the tensors u [bb, hu, wu, ca] and v [bb, hv, wv, cb] (pixel strides uld, vld), scattered to dw[a * s_a + b * s_b + tap] (flip: taps reversed).  The
    fields are the arguments of rv_conv_wgrad and its deferred / segmented forms; mode 0: 3x3, 1: 1x1, 2: 2x2 stride 2, | 0x100: bf16 operands."""
    __slots__ = ()

    # what the library keys its partition and its workspace size by (rv_conv_wgrad_set_plan, rv_conv_wgrad_workspace_bytes: no row width) / the tuner and the plan table
    plan_key = property(lambda self: (self.taps, self.bb, self.hv, self.ca, self.cb))
    tune_key = property(lambda self: (self.taps, self.bb, self.hv, self.wv, self.ca, self.cb))

    def same_geometry(self, other):
        """Equal but for where the operands live: the two may be segments of one launch."""
        return self._replace(u=None, v=None) == other._replace(u=None, v=None)

    def head(self):
        """The leading arguments of rv_conv_wgrad / rv_conv_wgrad_deferred."""
        return self.mode, ptr(self.u), self.uld, self.hu, self.wu, self.ca, ptr(self.v), self.vld, self.hv, self.wv, self.cb, self.bb


def _wgrad_args(probs, dw, db, ws, nbytes, stream_ptr, acc=None, slot=None):
    """(entry point, its arguments, the objects the arguments point into) of ONE weight-gradient launch, the only place that knows the four argument
    lists.  One problem: rv_conv_wgrad; several (of the same geometry): the segmented form.  slot (a reduction-table entry): the deferred form, which
    always accumulates; else `acc`."""
    p, n = probs[0], len(probs)
    if n == 1:
        head, held = p.head(), None
    else:
        held = [(ctypes.c_void_p * n)(*[q.u.data_ptr() for q in probs]), (ctypes.c_void_p * n)(*[q.v.data_ptr() for q in probs])]
        head = (p.mode, n, ctypes.addressof(held[0]), ctypes.addressof(held[1]), p.uld, p.hu, p.wu, p.ca, p.vld, p.hv, p.wv, p.cb, p.bb)
    tail = (acc, ptr(ws), nbytes) if slot is None else (ptr(ws), nbytes, slot)
    name = 'rv_conv_wgrad' + ('' if slot is None else '_deferred') + ('' if n == 1 else '_seg')
    return name, head + (ptr(dw), p.s_a, p.s_b, p.flip, ptr(db)) + tail + (stream_ptr,), held


def _tune_wgrad(lib, p, w):
    """Per-shape partition of the MFMA weight-gradient kernel (waves per workgroup x workgroups on the chip): the plan table's, or the first eager call of a shape
    times the candidates (scratch outputs shaped like `w`) and pins the winner (rv_conv_wgrad_set_plan); under hipGraph capture an untuned shape keeps the library default."""
    key = p.tune_key
    taps, bb, hv, wv, ca, cb = key
    if not AUTOTUNE or ca * cb * taps <= 144 or ca == 1:
        return
    if AUTOTUNE == 'table' or key in tuning._wgrad_tuned:
        # (runs before the first launch of the shape, i.e. never between a deferred weight-gradient launch of that shape and its table flush)
        return tuning.wgrad_plan_for(lib, key, AUTOTUNE)
    if torch.cuda.is_current_stream_capturing():
        return tuning._repin_wgrad(lib, key)
    tuning._wgrad_tuned.add(key)
    st = torch.cuda.current_stream()
    dw = torch.empty_like(w)
    db = torch.empty(cb, device=w.device, dtype=torch.float32)
    held = []

    def try_plan(plan):
        if lib.rv_conv_wgrad_set_plan(*p.plan_key, *plan) != 0:
            return 1
        nbytes = lib.rv_conv_wgrad_workspace_bytes(*p.plan_key)
        ws = torch.empty(nbytes // 4, device=w.device, dtype=torch.float32)
        held[:] = [_wgrad_args([p._replace(mode=p.mode & 0xff)], dw, db, ws, nbytes, st.cuda_stream, acc=0)[1], ws]      # (timed with fp32 operands)
        return lib.rv_conv_wgrad(*held[0])
    choice = tuning.tune('wgrad', key, tuning.wgrad_candidates(taps, hv, winograd=os.environ.get('RV_TUNE_WGRAD_WINO', '1') != '0'), try_plan,
                         lambda plan: tuning.best_of_bursts(lambda: lib.rv_conv_wgrad(*held[0]), st), default=(0, 0),
                         describe=lambda c: f'taps={taps} {ca}->{cb} {hv}x{wv} B={bb}: nw={c[0]} wgs={c[1]}')
    tuning._pin_wgrad(lib, key, choice)
    tuning._wgrad_plans[key] = choice


def _wgrad_geom(kind, x, dy, bf16=False):
    """The WgradProblem of a conv layer's weight gradient.  Pure: shapes and strides in, record out (CPU tensors serve)."""
    bb, h, wd, cin, xld = _geom(x)
    _, ho, wo, cout, yld = _geom(dy)
    if kind == 'up':
        # G[tap][a=co][b=ci] = sum_p dY[2p+tap][co] * X[p][ci]  -> dWt[ci][co][tap]
        taps, mode = 4, 2
        u, uld, hu, wu, ca = dy, yld, ho, wo, cout
        v, vld, hv, wv, cb = x, xld, h, wd, cin
        s_a, s_b, flip = 4, cout * 4, 0
    else:
        mode, taps = {'c3': (0, 9), 't3': (0, 9), 'c1': (1, 1), 'down': (2, 4)}[kind]
        u, uld, hu, wu, ca = x, xld, h, wd, cin
        v, vld, hv, wv, cb = dy, yld, ho, wo, cout
        s_a, s_b, flip = (cout * 9, 9, 1) if kind == 't3' else (taps, cin * taps, 0)
        if bf16 and taps == 9:
            mode |= 0x100                       # bf16 operands on the matrix pipe (opt-in experiment, see BF16)
    return WgradProblem(mode, taps, u, uld, hu, wu, ca, v, vld, hv, wv, cb, bb, s_a, s_b, flip)


def _wgrad_launch(probs, dw, db, acc, st):
    """ONE weight-gradient launch on `st`, the current torch stream of dw's device: dw / db (+)= the sum over `probs` -- one WgradProblem, or the same
    layer's problems of several backward passes as the segments of one launch (those always accumulate).  Inside deferred_wgrad_reductions an
    accumulating launch only leaves its partial sums and registers the reduction with the stream's table -- unless the sums must be ordered
    (DETERMINISTIC), and never for the 1 -> many 3x3 layer.  False: the layer has no segmented form, nothing was launched (the caller launches per pass)."""
    p, n, lib = probs[0], len(probs), _lib.load()
    if n == 1:
        _tune_wgrad(lib, p, dw)
    elif not all(p.same_geometry(q) for q in probs):
        return False
    else:
        p = p._replace(bb=n * p.bb)
        if AUTOTUNE:
            # the partition of n * bb images: the table's entry (or the nearest batch's), else the one this process tuned for one pass -- never the
            # on-line tuner's timing launches (they read n * bb CONTIGUOUS images from the first segment)
            tuning.wgrad_plan_for(lib, p.tune_key, AUTOTUNE, probs[0].tune_key)
    nbytes = lib.rv_conv_wgrad_workspace_bytes(*p.plan_key)
    ws = torch.empty(nbytes // 4, device=dw.device, dtype=torch.float32)
    tab = None
    if _WGRAD_DEFER[0] is not None and acc and not DETERMINISTIC[0] and not (p.taps == 9 and p.ca == 1 and p.cb > 16):
        tab = _WGRAD_DEFER[0].table(st.cuda_stream, lambda: _WgradTable(dw.device, st))
    name, args, held = _wgrad_args(probs, dw, db, ws, nbytes, st.cuda_stream, acc, None if tab is None else tab.slot())
    rc = invoke(name, *args)
    if (rc != 0) if tab is None else (rc <= 0):
        if n > 1:
            return False
        raise RuntimeError(f'{name} failed ({rc}): {_lib.last_error()}')
    if tab is not None:
        tab.n += 1
        tab.keep.append(ws)
    return True


# one backward pass's weight gradient as WgradMerger parks it: dw / db are the buffers it adds into (db None: no bias gradient from this launch), stream the pass's torch stream
WgradItem = namedtuple('WgradItem', 'kind x dy w dw db bf16 stream')


def conv_wgrad(kind, x, dy, w, want_bias=True, dw_acc=None, db_acc=None, bf16=False, colsum=None):
    """(dw, db) in the PyTorch layouts of `w` / bias; with dw_acc/db_acc the results are ADDED into those buffers."""
    p = _wgrad_geom(kind, x, dy, bf16)
    cout = dy.shape[3]
    acc = 1 if dw_acc is not None else 0
    dw = dw_acc if acc else torch.empty_like(w)
    db = None if not want_bias else db_acc if acc else torch.empty(cout, device=w.device, dtype=torch.float32)
    bias = None if kind == 'up' else db              # (the up-conv's bias gradient is a column sum of dY: below)
    st = torch.cuda.current_stream(w.device)
    merger = _WGRAD_MERGE[0]
    if not (merger is not None and acc and not DETERMINISTIC[0] and p.ca > 2 and p.cb > 2 and
            merger.submit((_bucket_offset(dw.data_ptr()), p.mode), WgradItem(kind, x, dy, w, dw, bias, bf16, st))):
        _wgrad_launch([p], dw, bias, acc, st)        # (else: launched with the same layer's other passes of this step, WgradMerger)
    if kind == 'up' and want_bias:
        if colsum is not None and colsum.sums is not None:
            # dY's column sums came with the kernel that produced dY (ColsumLink): fold the replicas, no pass over dY
            call('rv_sums_fold', ptr(colsum.sums), colsum.c, 0, cout, ptr(db), acc, stream())
        else:
            _colsum_into(dy, dy.stride(2), p.bb * dy.shape[1] * dy.shape[2], cout, db, acc)
    return (None, None) if acc else (dw, db)


def conv_wgrad_merged(items):
    """ONE weight-gradient launch for the same layer's (x, dY) pairs of several backward passes (rv_conv_wgrad_seg: up to four segments of
    identical geometry).  items: WgradItems (or their tuples), all of one layer and one gradient buffer -- the first one's.  False: not launched."""
    first = WgradItem(*items[0])
    probs = [_wgrad_geom(it[0], it[1], it[2], first.bf16) for it in items]
    return len(probs) > 1 and _wgrad_launch(probs, first.dw, first.db, 1, torch.cuda.current_stream(first.w.device))


def _bucket_of(p_):
    """(is it the main bucket, offset in it) for a gradient pointer inside one of the chains' gradient buckets (the side chains add into twins of the flat
    bucket, SIDE_GRADS); None outside all of them."""
    if SIDE_GRADS[0] is not None:
        main, twins = SIDE_GRADS[0]
        for t in (main, *twins.values()):
            if t.data_ptr() <= p_ < t.data_ptr() + t.numel() * 4:
                return t is main, p_ - t.data_ptr()
    return None


def _bucket_offset(p_):
    """A gradient buffer's identity across the chains' gradient buckets: its offset inside whichever bucket holds it (no buckets: the pointer itself)."""
    hit = _bucket_of(p_) if (_WGRAD_MERGE_ACROSS and _WGRAD_MERGE_HELPER) else None
    return p_ if hit is None else hit[1]


def _in_main_bucket(p_):
    return (_bucket_of(p_) or (False,))[0]


# --------------------------------------------------------------------------------------------
# one weight-gradient launch per layer and STEP (per gradient bucket), not per backward pass
# --------------------------------------------------------------------------------------------
_WGRAD_MERGE = [None]
_WGRAD_MERGE_HELPER = os.environ.get('RV_WGRAD_MERGE_HELPER', '1') != '0'      # the main chain's merged launches run on the (then idle) side stream
_WGRAD_MERGE_ACROSS = os.environ.get('RV_WGRAD_MERGE_ACROSS', '1') != '0'      # the side chain's pass of a shared layer joins the main chain's launch
_WGRAD_MERGE_MAX = min(4, max(2, int(os.environ.get('RV_WGRAD_MERGE_MAX', '4'))))      # passes per launch (rv_conv_wgrad_seg takes up to four)


class WgradMerger:
    """The transcriber is back-propagated four times per training step (model/UNet_onset.py:383,117-146: the two VAT final passes, the
    reconstruction branch's second transcription, the main forward) and every pass launched its own weight-gradient kernel per layer.  A
    weight gradient is a sum over pixels, so the passes of one layer can be ONE launch over their (x, dY) pairs as segments
    (rv_conv_wgrad_seg) -- the fixed cost of such a launch (prologue, accumulator fold, partial sums, reduction entry: ~10 us of 35-60)
    is paid once: 4 x 49.9 -> 155 us for 64 -> 64 @160x57 at B = 8 per pass.
    * A layer is known by the OFFSET of its gradient in the gradient bucket, so the side chain's pass (which adds into a twin of the
      bucket) joins the main chain's; the sum goes to the main bucket.
    * How many passes a layer sees per step is LEARNED from a step that runs unmerged (per mode: one chain or two); afterwards a pass
      only registers its operands and the last one launches.  `finish()` launches whatever is still pending (a step that took another
      path) and re-learns the counts.
    * WHERE it launches decides whether it pays (profiles/r05_wgrad_merge_ab.txt): on the side stream, which is idle while the main chain
      runs the main forward's backward -- merged on the main chain the same launches LOSE 0.14 ms/step, next door they win 0.5.  The
      launching stream first waits for every other stream a segment was produced on.
    * Memory: the parked (x, dY) pairs of up to three passes stay alive until the last pass of a layer arrives: +0.8 GB of peak device memory at
      B = 8 + 8 (bench.py `device_memory_gb.max_allocated`: 6.28 GB merged, 5.48 GB per pass; 7.9 GB reserved either way) -- 0.3 % of the 288 GB of
      an MI355X, so there is no budget gate; an exception inside the step drops the parked references (`abort`)."""

    def __init__(self):
        self.learned = {}          # (mode, key) -> launches per step
        self.mode = None
        self.counts, self.pending = {}, {}
        self.merged_launches = 0   # segmented launches of the current step (0 in a learning step)
        self.seen = set()          # modes whose pass counts have been learned (a finished step of that mode)

    def begin(self, mode):
        self.mode, self.counts, self.pending, self.merged_launches = mode, {}, {}, 0

    def knows(self, mode):
        """True once a step of this mode (one chain / two chains) has run unmerged, i.e. the next step of that mode merges."""
        return mode in self.seen

    def abort(self):
        """An exception left the step: drop the parked (x, dY) references instead of pinning them until the next step."""
        self.pending, self.counts = {}, {}

    def submit(self, key, item):
        self.counts[key] = self.counts.get(key, 0) + 1
        want = self.learned.get((self.mode, key))
        if want is None or want < 2:
            return False                           # learning step / single pass: the caller launches now
        q = self.pending.setdefault(key, [])
        q.append(item)
        if len(q) >= min(want, _WGRAD_MERGE_MAX):
            self._launch(key)
        return True

    def _launch(self, key):
        q = self.pending.pop(key, [])
        if not q:
            return
        q.sort(key=lambda it: not _in_main_bucket(it.dw.data_ptr()))       # the sum goes to the main chain's bucket when one of the passes is its
        dev = q[0].w.device
        cur = torch.cuda.current_stream(dev)
        where = self._helper_for(q) or cur
        # the last pass of the main chain (the main forward's backward) runs while the side chain is idle: its input-gradient chain stays
        # there, the merged weight gradients go next door (they ADD into the main bucket through the reduction table's atomics).  Whatever
        # stream launches: it first waits for every OTHER stream a pass of the group was produced on.
        origins = {it.stream.cuda_stream: it.stream for it in q}
        with torch.cuda.stream(where):
            for sp, st in origins.items():
                if sp != where.cuda_stream:
                    ev = torch.cuda.Event()
                    ev.record(st)
                    where.wait_event(ev)
            for it in q:
                if it.stream.cuda_stream != where.cuda_stream:
                    it.x.record_stream(where)
                    it.dy.record_stream(where)
            self._launch_here(q)

    def _helper_for(self, q):
        if not _WGRAD_MERGE_HELPER or len(q) < 2 or not DUAL_STREAM[0] or _WGRAD_DEFER[0] is None or not _in_main_bucket(q[0].dw.data_ptr()) or not SIDE_GRADS[0][1]:
            return None
        dev = q[0].w.device
        helper = side_stream(dev, 0)
        if helper.cuda_stream == torch.cuda.current_stream(dev).cuda_stream:
            return None
        return helper

    def _launch_here(self, q):
        # passes of different geometry (the labelled and the unlabelled batch may differ in size) merge among their likes
        groups = {}
        for it in q:
            groups.setdefault((tuple(it.x.shape), it.x.stride(), tuple(it.dy.shape), it.dy.stride()), []).append(it)
        dw0, db0 = q[0].dw, q[0].db                # (every launch of the group adds into the first item's buffers: the main chain's when it has a pass)
        for g in groups.values():
            g = [it._replace(dw=dw0, db=db0 if it.db is not None else None) for it in g]
            if len(g) >= 2 and conv_wgrad_merged(g):
                self.merged_launches += 1
                continue
            merger, _WGRAD_MERGE[0] = _WGRAD_MERGE[0], None
            try:
                for it in g:                           # a single pass, or no segmented form for this layer: per pass after all
                    conv_wgrad(it.kind, it.x, it.dy, it.w, it.db is not None, it.dw, it.db, bf16=it.bf16)
            finally:
                _WGRAD_MERGE[0] = merger

    def finish(self):
        for key in list(self.pending):
            self._launch(key)
        for key, n in self.counts.items():
            self.learned[(self.mode, key)] = n
        self.seen.add(self.mode)


class wgrad_merging:
    def __init__(self, merger, mode):
        self.merger, self.mode = merger, mode

    def __enter__(self):
        self.prev = _WGRAD_MERGE[0]
        _WGRAD_MERGE[0] = self.merger
        if self.merger is not None:
            self.merger.begin(self.mode)
        return self.merger

    def __exit__(self, exc_type, *exc):
        _WGRAD_MERGE[0] = self.prev
        if exc_type is not None and self.merger is not None:
            self.merger.abort()


# --------------------------------------------------------------------------------------------
# deferred weight-gradient reductions: one table-driven launch per stream and backward pass
# --------------------------------------------------------------------------------------------
_WGRAD_DEFER = [None]
_WGRAD_POOL = []           # pre-allocated pinned host tables for hipGraph capture (never recycled once captured)
_WGRAD_KEEP = []
_WGRAD_MAX = 512           # entries per table


def prepare_wgrad_tables(n=3):
    """Pinned host tables for deferred_wgrad_reductions under hipGraph capture (call outside capture)."""
    _fill_pool(_WGRAD_POOL, n, _WGRAD_MAX * _lib.load().rv_wgrad_table_entry_bytes())


class _WgradTable(_HostTable):
    def __init__(self, device, torch_stream):
        super().__init__('deferred_wgrad_reductions', _lib.load().rv_wgrad_table_entry_bytes(), _WGRAD_MAX, _WGRAD_POOL, _WGRAD_KEEP, torch_stream)
        self.keep = []

    def flush(self):
        if self.n == 0:
            return
        n, total = self.n, _lib.load().rv_wgrad_table_finalize(self.host.data_ptr(), self.n)
        with torch.cuda.stream(self.stream):
            call('rv_wgrad_reduce_table', ptr(self.upload()), n, total, self.stream.cuda_stream)
        self.keep = []


class _deferred:
    """Base of the deferred_* contexts: while active, the module's one-element list `slot` exposes the context, whose {key: table} dict the launches fill."""

    def __enter__(self):
        self.prev = self.slot[0]
        self.tables = {}
        self.slot[0] = self
        return self

    def __exit__(self, *exc):
        self.slot[0] = self.prev

    def table(self, key, make):
        """The table under `key` (a stream, or a stream and more), made on first use."""
        if key not in self.tables:
            self.tables[key] = make()
        return self.tables[key]

    def flush(self):
        for t in self.tables.values():
            t.flush()


class deferred_wgrad_reductions(_deferred):
    """While active, conv weight-gradient calls that accumulate into param.grad launch only their partial-sum kernel; the
    reductions of ALL layers run as one launch per stream at ``flush()`` (call it after backward, before the gradients are
    read).  One reduction launch per layer is launch-latency bound (161 launches of ~5 us per step)."""
    slot = _WGRAD_DEFER


def _out_hw(kind, h, w, size):
    if kind == 'down':
        return h // 2, w // 2
    if kind == 'up':
        return (2 * h, 2 * w) if size is None else (int(size[0]), int(size[1]))
    return h, w


# A conv layer's weight gradient is launched BEFORE its input gradient in the backward (RV_WGRAD_FIRST=0: the other way round).  The input
# gradient is the one the next layer's backward waits for, so "input gradient first" looks right -- measured in situ it is the slower order
# (tools/knob_ab.sh, round 5: 21.30 vs 21.48 ms/step): both kernels read dY, and the weight-gradient kernel's single pass over X and dY leaves
# dY in the cache hierarchy for the input-gradient kernel that follows, whose output the next layer then finds warm.  Results are unaffected.
WGRAD_FIRST = [os.environ.get('RV_WGRAD_FIRST', '1') != '0']
_WGRAD_FIRST_UPCAT = os.environ.get('RV_WGRAD_FIRST_UPCAT', '1') != '0'      # (the decoder's up-conv + skip-conv pair follows the same order)


def _conv_param_grads(kind, x, dy, w, params, need_b, dy_colsum=None, bf16=False):
    """The weight-gradient half of a conv layer's backward: (dw, db) for autograd, or (None, None) when they were added straight into the .grad of
    `params` = (weight, bias) -- direct_param_grads, and only when every gradient that is wanted has a buffer there: the weight's, and the bias's unless
    need_b is False."""
    gw, gb = _grad_buf(params[0]), _grad_buf(params[1])
    if gw is None or (gb is None and need_b):
        gw = gb = None
    return conv_wgrad(kind, x, dy, w, need_b, gw, gb, bf16=bf16, colsum=dy_colsum)


def _conv_input_grad(kind, dy, w, xshape, share=None, bn_in=None, dx_colsum=None, bf16=False):
    """The input-gradient half: dx, or None when it was added into the GradShare's buffer (a later consumer of a shared input).  bn_in: see
    conv_dgrad_into (it owns the kernel's epilogue: no GradShare, no column sums then); dx_colsum: a ColsumLink to leave the column sums of dx in."""
    if share is not None and bn_in is None:
        return share.dgrad(kind, dy, w, xshape, bf16=bf16)
    dx = torch.empty(xshape, device=dy.device, dtype=torch.float32)
    sum_ws = ARENA.take(bn_ws_doubles(xshape[3]), dy.device) if (dx_colsum is not None and bn_in is None) else None
    conv_dgrad_into(kind, dy, w, dx, bn_in, bf16=bf16, sum_ws=sum_ws)
    if sum_ws is not None:
        dx_colsum.sums, dx_colsum.c = sum_ws, xshape[3]
    return dx


def _conv_backward(kind, x, dy, w, params, need_x, need_w, need_b, *, xshape, share=None, bn_in=None, dx_colsum=None, dy_colsum=None, bf16=False,
                   wgrad_first=None):
    """One conv layer's backward, (dx, dw, db): its two halves in the order of WGRAD_FIRST (wgrad_first overrides).  dx_colsum is only filled in a
    final graph (live weights: need_w); dy_colsum (kind 'up': the column sums of dy, the bias gradient) is released afterwards."""
    dx = dw = db = None
    for weights in ((True, False) if (WGRAD_FIRST[0] if wgrad_first is None else wgrad_first) else (False, True)):
        if weights and need_w:
            dw, db = _conv_param_grads(kind, x, dy, w, params, need_b, dy_colsum, bf16)
        elif not weights and need_x:
            dx = _conv_input_grad(kind, dy, w, xshape, share, bn_in, dx_colsum if need_w else None, bf16)
    if dy_colsum is not None:
        dy_colsum.sums = None            # drop the reference
    return dx, dw, db


class ConvFn(Function):
    """y = conv(x) for any of the five conv kinds (new contiguous NHWC tensor)."""

    @staticmethod
    def forward(ctx, x, w, b, kind, size, stats=None, bn_in=None, share=None, dx_colsum=None, dy_colsum=None):
        """dx_colsum: a ColsumLink this conv's input-gradient kernel fills (column sums of dx); dy_colsum: a filled-in-backward
        ColsumLink holding the column sums of this conv's dY (kind 'up': its bias gradient)."""
        bb, h, wd, cin, _ = _geom(x)
        _, cout = _channels(kind, w)
        ho, wo = _out_hw(kind, h, wd, size)
        y = _new(bb, ho, wo, cout, x)
        ctx.live = bool(ctx.needs_input_grad[1])       # live weights <=> a final graph (bf16_final_graphs applies to those only)
        conv_forward_into(kind, x, w, b, y, stats, bf16=BF16['fwd'] and ctx.live)
        ctx.kind = kind
        ctx.xshape = tuple(x.shape)
        ctx.bn_in = bn_in            # BnLink of the BatchNorm whose output is x (single consumer), or None
        ctx.share = share            # GradShare of x (several conv consumers), or None
        ctx.dx_colsum, ctx.dy_colsum = dx_colsum, dy_colsum
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, w)
        ctx.params = (w, b)          # parameter objects (for direct gradient accumulation)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        return _conv_backward(ctx.kind, x, dy.contiguous(), w, ctx.params, *ctx.needs_input_grad[:3], xshape=ctx.xshape, share=ctx.share, bn_in=ctx.bn_in,
                              dx_colsum=ctx.dx_colsum, dy_colsum=ctx.dy_colsum, bf16=BF16['bwd'] and ctx.live) + (None,) * 7


class UpCatFn(Function):
    """cat = concat(up(x, output_size), conv3x3(skip_src)) along channels, written in place into one NHWC
    buffer (d_block.forward's `self.us(x, output_size=size)` + `torch.cat((x, skip), 1)`,
    model/UNet_onset.py:219-220, with the encoder's extra skip conv, :244-246, computed here)."""

    @staticmethod
    def forward(ctx, x, w_up, b_up, s, w_skip, b_skip, size, share=None, dy_colsum=None):
        bb, h, wd, cin, _ = _geom(x)
        cu = w_up.shape[1]
        cs = w_skip.shape[0]
        ho, wo = int(size[0]), int(size[1])
        cat = _new(bb, ho, wo, cu + cs, x)
        ctx.live = bool(ctx.needs_input_grad[1] or ctx.needs_input_grad[4])
        conv_forward_into('up', x, w_up, b_up, cat[..., :cu])
        conv_forward_into('c3', s, w_skip, b_skip, cat[..., cu:], bf16=BF16['fwd'] and ctx.live)
        ctx.cu = cu
        ctx.dy_colsum = dy_colsum    # ColsumLink: column sums of dcat from the kernel that produces it
        ctx.share = share            # GradShare of s (it also feeds the next encoder block)
        ctx.shapes = (tuple(x.shape), tuple(s.shape))
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[4]
        ctx.save_for_backward(x if need_w else None, s if need_w else None, w_up, w_skip)
        ctx.params = (w_up, b_up, w_skip, b_skip)
        return cat

    @staticmethod
    def backward(ctx, dcat):
        x, s, w_up, w_skip = ctx.saved_tensors
        dcat = dcat.contiguous()
        cu = ctx.cu
        d_up, d_sk = dcat[..., :cu], dcat[..., cu:]
        pwu, pbu, pws, pbs = ctx.params
        need_x, need_wu, _, need_s, need_ws = ctx.needs_input_grad[:5]
        bf = BF16['bwd'] and ctx.live
        dx = ds = dwu = dbu = dws = dbs = None
        # two conv layers, their halves interleaved: BOTH weight gradients (the up conv's with its bias fold first), then both input gradients, or
        # the reverse.  Both bias gradients are always computed (need_b = True, whatever autograd asks for), so the one direct-gradient rule applies.
        for weights in ((True, False) if (WGRAD_FIRST[0] and _WGRAD_FIRST_UPCAT) else (False, True)):
            if weights and need_wu:
                dwu, dbu = _conv_param_grads('up', x, d_up, w_up, (pwu, pbu), True, ctx.dy_colsum)
            if weights and need_ws:
                dws, dbs = _conv_param_grads('c3', s, d_sk, w_skip, (pws, pbs), True, bf16=bf)
            if not weights and need_x:
                dx = _conv_input_grad('up', d_up, w_up, ctx.shapes[0])
            if not weights and need_s:
                ds = _conv_input_grad('c3', d_sk, w_skip, ctx.shapes[1], ctx.share, bf16=bf)
        if ctx.dy_colsum is not None:
            ctx.dy_colsum.sums = None
        return dx, dwu, dbu, ds, dws, dbs, None, None, None


# --------------------------------------------------------------------------------------------
# BatchNorm (train / eval) + leaky ReLU (+ residual)
# --------------------------------------------------------------------------------------------
def skip_conv_ksplit(x, cout):
    """Which arithmetic the SEPARATE launch of the 1x1 skip conv x -> cout channels would use (the fused form inside the BatchNorm apply kernel must reproduce it bit
    for bit): False = one fmaf chain over the input channels (conv_small_k for one input channel; conv_mfma_k's plain tiles), True = the K-split tile family 0x5NM
    (four partial chains added in wave order), None = unknown -- on-line tuning, a forced algo, a table entry borrowed from another batch size, or an input that the
    fused kernel does not take -- in which case the caller keeps the separate launch."""
    bb, h, wd, cin, ild = _geom(x)
    if cin == 1:
        return False
    if cin not in (16, 32, 64) or ild % 4 or x.data_ptr() % 16 or os.environ.get('RV_FORCE_ALGO_ALL'):
        return None
    if AUTOTUNE is False:
        return False                         # library default tile: choose_tiles, never the K-split family
    if AUTOTUNE != 'table':
        return None
    hit = plans.lookup_conv((1, bb, h, wd, cin, cout, ild, cout, False, False))
    if hit is None:
        return False                         # not in the table: library default tile
    if not hit[1]:
        return None                          # borrowed from another batch size: its legality is only known after the first launch
    return tuning.decode(hit[0])[0] in tuning.KSPLIT_FAMILIES


class BnActFn(Function):
    """y = leaky_relu(batch_norm(z)) (+ res).  Training mode updates running_mean / running_var /
    num_batches_tracked in place exactly like nn.BatchNorm2d(momentum=0.1)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, nbt, res, training, slope, stats=None, link=None,
                r1_x=None, r1_w=None, r1_b=None, r1_share=None):
        """r1_x / r1_w / r1_b (round 6): the residual as a RANK-1 term -- skip(x) of the first encoder block, a 1 -> C 1x1 conv of the single-channel
        input (model/UNet_onset.py:191,198) -- evaluated inside the apply kernel (rv_bn_lrelu_fwd_skip; 16 / 32 / 64-channel inputs: the dense form, opt-in) instead of a conv launch writing it and this kernel
        reading it back; the backward launches that conv's input / weight gradients from dy exactly as ConvFn.backward would (r1_share: the GradShare of x)."""
        need_gpu(z, gamma)
        bb, h, wd, c, zld = _geom(z)
        p = bb * h * wd
        y = torch.empty_like(z, memory_format=torch.contiguous_format)
        coef = torch.empty(5 * c, device=z.device, dtype=torch.float32)
        mode = 1 if training else 0
        if training and _BN_DEFER[0] is not None:
            mode = 2
            _BN_DEFER[0].append((running_mean, running_var, nbt, coef, c))
        # zero-initialised fp64 sums: one slice for the forward statistics, one for the backward reduction
        # (``stats``: the producing conv already left the forward sums in its slice -- bn_stats_slot / ConvFn)
        ready = training and stats is not None
        ws = (stats if ready else ARENA.take(bn_ws_doubles(c), z.device),
              ARENA.take(bn_ws_doubles(c), z.device) if (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) else None)
        rld = _geom(res)[4] if res is not None else 0
        ctx.r1 = r1_x is not None
        if ctx.r1:
            cin1 = r1_x.shape[-1]
            assert res is None and tuple(r1_x.shape[:3]) == (bb, h, wd) and r1_w.shape[0] == c and r1_w.numel() == c * cin1 and r1_w.is_contiguous()
            need_gpu(r1_x, r1_w)
            ks = skip_conv_ksplit(r1_x, c)
            assert ks is not None, 'fused skip conv: the tile of the separate launch is not known (ops.fusable_skip decides)'
            call('rv_bn_lrelu_fwd_skip', ptr(z), zld, p, c, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), ptr(nbt),
                 BN_MOMENTUM, BN_EPS, mode, slope, ptr(r1_x), _geom(r1_x)[4], cin1, ptr(r1_w), ptr(r1_b), 1 if ks else 0, ptr(y), c, ptr(coef), ptr(ws[0]),
                 1 if ready else 0, stream())
            ctx.r1_share, ctx.r1_xshape, ctx.r1_params = r1_share, tuple(r1_x.shape), (r1_w, r1_b)
            ctx.r1_live = bool(ctx.needs_input_grad[12])
        else:
            call('rv_bn_lrelu_fwd', ptr(z), zld, p, c, ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), ptr(nbt),
                 BN_MOMENTUM, BN_EPS, mode, slope, ptr(res), rld, ptr(y), c, ptr(coef), ptr(ws[0]), 1 if ready else 0, stream())
        ctx.ws = ws
        ctx.link = None
        if link is not None and training and ws[1] is not None and res is None and not ctx.r1:
            link.z, link.coef, link.ws, link.slope, link.ready = z, coef, ws[1], slope, False
            ctx.link = link
        ctx.training = training
        ctx.slope = slope
        ctx.params = (gamma, beta)
        if ctx.r1:
            ctx.save_for_backward(z, coef, r1_x if ctx.needs_input_grad[12] else None, r1_w)
        else:
            ctx.save_for_backward(z, coef)
        return y

    @staticmethod
    def backward(ctx, dy):
        if ctx.r1:
            z, coef, r1_x, r1_w = ctx.saved_tensors
        else:
            z, coef = ctx.saved_tensors
        dy = dy.contiguous()
        dx1 = dw1 = db1 = None
        if ctx.r1:
            # the skip conv's own backward (ConvFn.backward of a 'c1' conv with input x, output gradient dy), launched here: it used to be
            # the first node behind this one on the residual path, so the order of the adds into x's shared gradient is unchanged
            dx1, dw1, db1 = _conv_backward('c1', r1_x, dy, r1_w, ctx.r1_params, *ctx.needs_input_grad[11:14], xshape=ctx.r1_xshape, share=ctx.r1_share)
        bb, h, wd, c, zld = _geom(z)
        p = bb * h * wd
        need_w = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dz = torch.empty_like(z, memory_format=torch.contiguous_format)
        pg, pb = ctx.params
        gg, gb = (_grad_buf(pg), _grad_buf(pb)) if need_w else (None, None)
        direct = gg is not None and gb is not None
        if direct:
            dg, db = gg, gb
        else:
            dg = torch.empty(c, device=z.device, dtype=torch.float32) if need_w else None
            db = torch.empty(c, device=z.device, dtype=torch.float32) if need_w else None
        ready = ctx.link is not None and ctx.link.ready      # the consumer conv's dgrad already reduced (dy, z)
        call('rv_bn_lrelu_bwd', ptr(dy), c, ptr(z), zld, p, c, ptr(coef), ctx.slope, 0 if ctx.training else 1,
             ptr(dz), c, ptr(dg), ptr(db), 1 if direct else 0,
             ptr(ctx.ws[1] if ctx.ws[1] is not None else ARENA.take(bn_ws_doubles(c), z.device)), 1 if ready else 0, stream())
        if ctx.link is not None:
            ctx.link.z = ctx.link.coef = ctx.link.ws = None   # drop the references
        if direct:
            dg = db = None
        dres = dy if ctx.needs_input_grad[6] else None
        return (dz if ctx.needs_input_grad[0] else None), dg, db, None, None, None, dres, None, None, None, None, dx1, dw1, db1, None


# --------------------------------------------------------------------------------------------
# linear layers
# --------------------------------------------------------------------------------------------
def _mat(t):
    """(ptr, rows, cols, row stride, col stride) of a 2-D view."""
    assert t.dim() == 2
    return ptr(t), t.shape[0], t.shape[1], t.stride(0), t.stride(1)


def _splitk_for(m_out, n_out, k):
    """Library-default split-K heuristic (shapes outside the plan table): enough workgroups to cover the chip twice."""
    blocks = ((m_out + 63) // 64) * ((n_out + 63) // 64)
    if blocks >= 256 or k < 512:
        return 1
    return max(1, min(16, 512 // blocks, k // 128))


def gemm(a, b_kn, c, bias=None, act=0, accumulate=False, splitk=None, c2=None, batch=1, bstrides=(0, 0, 0), a_rowsum=None,
         deterministic=True, defer_ok=False):
    """c[m,n] (+)= act(sum_k a[m,k] * b_kn[k,n] + bias[n]) on arbitrary 2-D views.  batch > 1: `batch` problems of this
    shape, problem z offset by z * bstrides (elements) from a / b_kn / c.  splitk None: the shipped plan table's factor for this
    shape (ops.AUTOTUNE == 'table'), the on-line tuner's (True), else the library heuristic; the reduction over k slices is
    folded in order inside the kernel (deterministic=True: forward / input-gradient chains, whose results feed the chaotic VAT
    direction and must be reproducible) or accumulated by fp32 atomics (deterministic=False: parameter gradients; faster)."""
    need_gpu(a, b_kn, c)
    pa, m, k, sam, sak = _mat(a)
    pb, k2, n, sbk, sbn = _mat(b_kn)
    pc, m2, n2, scm, scn = _mat(c)
    assert k == k2 and m == m2 and n == n2, (a.shape, b_kn.shape, c.shape)
    if c2 is not None:
        pc2, _, _, s2m, s2n = _mat(c2)
    else:
        pc2, s2m, s2n = None, 0, 0
    lib = _lib.load()

    def launch(s, pc_=pc, rs=ptr(a_rowsum), raise_=True):
        ws = tk = None
        if s > 1 and deterministic:
            # deterministic split-K: partial tiles are parked in `ws`, a second launch folds them in k order and runs the epilogue
            ws = torch.empty(lib.rv_gemm_splitk_workspace_bytes(m, n, s, batch) // 4, device=c.device, dtype=torch.float32)
        call('rv_gemm', pa, sam, sak, pb, sbk, sbn, pc_, scm, scn, pc2, s2m, s2n, ptr(bias), m, n, k, act,
             1 if accumulate else 0, s, batch, bstrides[0], bstrides[1], bstrides[2], rs, ptr(ws), ptr(tk), stream())

    deferrable = defer_ok and accumulate and not deterministic and bias is None and act == 0 and c2 is None and _GEMM_DEFER[0] is not None
    if splitk is None:
        key = (m, n, k, batch, int(sak <= sam), int(sbk <= sbn), act, int(bool(accumulate)) + 2 * int(bool(deterministic)))
        splitk = tuning._gemm_splitk.get(key)
        if splitk is None:
            if AUTOTUNE == 'table':
                splitk = plans.lookup_gemm(key)
            elif AUTOTUNE and c2 is None and not torch.cuda.is_current_stream_capturing():
                # time on scratch outputs: the real C may be a gradient that is being accumulated into
                extent = (m - 1) * scm + (n - 1) * scn + 1 + (batch - 1) * bstrides[2]
                tmp = torch.zeros(extent, device=c.device, dtype=torch.float32)
                rs_tmp = torch.zeros(m, device=c.device, dtype=torch.float32) if a_rowsum is not None else None
                # (split-K is deterministic for a given factor -- in-order fold --, so the choice only fixes the summation grouping)
                cands = tuning.gemm_splitk_candidates(m, n, k, (1, 2, 3, 4, 6, 8, 12, 16, 24, 32) if (deterministic or act == 0) else (1,))
                st = torch.cuda.current_stream()
                splitk = tuning.tune('gemm', key, cands, lambda s: launch(s, ptr(tmp), ptr(rs_tmp)) or 0,
                                     lambda s: tuning.best_of_bursts(lambda: launch(s, ptr(tmp), ptr(rs_tmp)), st),
                                     tuning.faster_by_3_percent, default=1, describe=lambda s: f'{key}: splitk={s}')
            if splitk is None:
                splitk = _splitk_for(m, n, k)
            tuning._gemm_splitk[key] = splitk
    if deferrable and _defer_gemm(a, b_kn, c, splitk, batch, bstrides, a_rowsum):
        return
    launch(splitk)


# --------------------------------------------------------------------------------------------
# deferred parameter-gradient GEMMs: one grouped launch per stream and backward pass
# --------------------------------------------------------------------------------------------
_GEMM_DEFER = [None]
_GEMM_POOL = []            # pre-allocated pinned host tables for hipGraph capture (never recycled once captured)
_GEMM_KEEP = []
_GEMM_MAX = 64             # entries per table (rv_gemm_table_run's scan limit)
KEEP_TABLES = [False]      # measurement mode (bench.py): flushed device tables and their operands stay alive for re-launching
GEMM_TABLE_WORK = {}       # device table pointer -> (flops, algorithmic bytes) of the grouped launch (filled in measurement mode)


def prepare_gemm_tables(n=3):
    """Pinned host tables for deferred_param_gemms under hipGraph capture (call outside capture)."""
    _fill_pool(_GEMM_POOL, n, _GEMM_MAX * _lib.load().rv_gemm_table_entry_bytes())


class _GemmTable(_HostTable):
    """The pending accumulating GEMMs of one (stream, operand orientation)."""

    def __init__(self, device, torch_stream, orientation):
        super().__init__('deferred_param_gemms', _lib.load().rv_gemm_table_entry_bytes(), _GEMM_MAX, _GEMM_POOL, _GEMM_KEEP, torch_stream)
        self.orientation, self.keep = orientation, []
        self.flops = self.bytes = 0.0

    def flush(self):
        if self.n == 0:
            return
        fold = ctypes.c_long(0)
        n, total = self.n, _lib.load().rv_gemm_table_finalize(self.host.data_ptr(), self.n, ctypes.addressof(fold))
        with torch.cuda.stream(self.stream):
            table = self.upload()
            call('rv_gemm_table_run', ptr(table), n, total, fold.value, self.orientation, self.stream.cuda_stream)
            if KEEP_TABLES[0]:
                _GEMM_KEEP.append((table, self.keep))
                GEMM_TABLE_WORK[table.data_ptr()] = (self.flops, self.bytes)
        self.keep = []
        self.flops = self.bytes = 0.0


class deferred_param_gemms(_deferred):
    """While active, linear-layer / attention parameter-gradient GEMMs that accumulate into param.grad are only REGISTERED; all of
    them run as one grouped launch per stream at ``flush()`` (after backward, before the gradients are read).  Alone each of them
    is a few dozen workgroups with a 5 120-long reduction: latency-bound, 25-90 us; side by side they fill the chip."""
    slot = _GEMM_DEFER


_TABLE_PARK = os.environ.get('RV_GEMM_TABLE_PARK', '1') != '0'      # (0: every k slice of a grouped GEMM adds atomically, the form until round 5)


def _defer_gemm(a, b_kn, c, splitk, batch, bstrides, a_rowsum):
    """Register c += a @ b_kn (atomic split-K) with the active deferred_param_gemms context; False if none is active."""
    if _GEMM_DEFER[0] is None:
        return False
    pa, m, k, sam, sak = _mat(a)
    pb, _, n, sbk, sbn = _mat(b_kn)
    pc, _, _, scm, scn = _mat(c)
    cur = torch.cuda.current_stream(c.device)
    orient = (1 if sak <= sam else 0) | (2 if sbk <= sbn else 0)
    tab = _GEMM_DEFER[0].table((cur.cuda_stream, orient), lambda: _GemmTable(c.device, cur, orient))
    if tab.n >= tab.capacity:
        return False
    lib = _lib.load()
    # split-K inside the grouped launch: slices parked in a per-entry workspace, folded by the table's second launch (one atomic per element)
    ws = torch.empty(lib.rv_gemm_splitk_workspace_bytes(m, n, splitk, batch) // 4, device=c.device, dtype=torch.float32) \
        if (splitk > 1 and _TABLE_PARK) else None
    rc = lib.rv_gemm_table_fill(tab.slot(), pa, sam, sak, pb, sbk, sbn, pc, scm, scn, None, m, n, k,
                                splitk, batch, bstrides[0], bstrides[1], bstrides[2], ptr(a_rowsum), ptr(ws))
    if rc < 0:
        raise RuntimeError(f'rv_gemm_table_fill failed ({rc}): {_lib.last_error()}')
    assert rc == orient
    tab.n += 1
    tab.flops += 2.0 * m * n * k * batch
    tab.bytes += 4.0 * batch * (m * k + k * n + m * n)
    tab.keep += [a, b_kn, c, a_rowsum, ws]      # operands stay alive (and their memory un-reused) until the grouped launch
    return True


def colsum(x2d, out=None, accumulate=False):
    if out is None:
        out = torch.empty(x2d.shape[1], device=x2d.device, dtype=torch.float32)
    assert x2d.stride(1) == 1
    _colsum_into(x2d, x2d.stride(0), x2d.shape[0], x2d.shape[1], out, accumulate)
    return out


def _colsum_into(x, ld, m, n, out, accumulate):
    if DETERMINISTIC[0]:
        ws = torch.empty(_lib.load().rv_colsum_ordered_workspace_bytes(m, n) // 4, device=out.device, dtype=torch.float32)
        call('rv_colsum_ordered', ptr(x), ld, m, n, ptr(out), 1 if accumulate else 0, ptr(ws), stream())
    else:
        call('rv_colsum', ptr(x), ld, m, n, ptr(out), 1 if accumulate else 0, stream())


def _param_wgrad(a_t, b, param, splitk=None, bias_param=None):
    """d(param) = a_t @ b.  Under direct_param_grads() the product is accumulated straight into param.grad (split-K
    atomics add onto it: no zero fill, no temporary, no autograd add) and None is returned.  bias_param: the layer's
    bias -- its gradient (the row sums of a_t = dY^T) then rides on the same GEMM; returns (None, True) in that case."""
    g = _grad_buf(param)
    if bias_param is not None:
        gb = _grad_buf(bias_param)
        if g is not None and gb is not None:
            gemm(a_t, b, g.view(a_t.shape[0], b.shape[1]), accumulate=True, splitk=splitk, a_rowsum=gb, deterministic=DETERMINISTIC[0], defer_ok=True)
            return None, True
        return _param_wgrad(a_t, b, param, splitk), False
    if g is not None:
        gemm(a_t, b, g.view(a_t.shape[0], b.shape[1]), accumulate=True, splitk=splitk, deterministic=DETERMINISTIC[0], defer_ok=True)
        return None
    dw = torch.empty((a_t.shape[0], b.shape[1]), device=b.device, dtype=torch.float32)
    gemm(a_t, b, dw, splitk=splitk, deterministic=DETERMINISTIC[0])
    return dw.view_as(param)


def _param_bgrad(dz2d, param):
    g = _grad_buf(param)
    if g is not None:
        colsum(dz2d, g, accumulate=True)
        return None
    return colsum(dz2d)


class LinearFn(Function):
    """y = act(x @ w.T + b) for a 2-D (possibly strided) x; act in {0: none, 1: sigmoid}."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        m, k = x.shape
        n = w.shape[0]
        y = torch.empty((m, n), device=x.device, dtype=torch.float32)
        gemm(x, w.t(), y, b, act)
        ctx.act = act
        ctx.params = (w, b)
        ctx.save_for_backward(x, w, y if act == 1 else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = dy.contiguous()
        m, k = x.shape
        n = w.shape[0]
        if ctx.act == 1:
            dz = torch.empty_like(dy)
            call('rv_sigmoid_bwd', ptr(dy), n, None, 0, ptr(y), n, ptr(dz), n, m, n, stream())
        else:
            dz = dy
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((m, k), device=dy.device, dtype=torch.float32)
            gemm(dz, _lin_t(w).t(), dx)
        bias_done = False
        if ctx.needs_input_grad[1]:
            if ctx.needs_input_grad[2]:
                dw, bias_done = _param_wgrad(dz.t(), x, ctx.params[0], None, ctx.params[1])
            else:
                dw = _param_wgrad(dz.t(), x, ctx.params[0], None)
        if ctx.needs_input_grad[2] and not bias_done:
            db = _param_bgrad(dz, ctx.params[1])
        return dx, dw, db, None


class OnsetHeadsFn(Function):
    """Spec2Roll's two heads + concat (model/UNet_onset.py:307-312):
         onset = sigmoid(linear_onset(y[..., 0])); feat = linear_feature(y[..., 1]); cat = [onset | feat]
       y: decoder output NHWC [B, T, 229, 2].  Returns (cat [B*T, 176], onset [B*T, 88])."""

    @staticmethod
    def forward(ctx, y, wo, bo, wf, bf):
        bb, t, nb, c = y.shape
        assert c == 2 and y.is_contiguous()
        m = bb * t
        y2 = y.view(m, nb, 2)
        cat = torch.empty((m, 176), device=y.device, dtype=torch.float32)
        onset = torch.empty((m, 88), device=y.device, dtype=torch.float32)
        gemm(y2[..., 0], wo.t(), cat[:, :88], bo, act=1, c2=onset)
        gemm(y2[..., 1], wf.t(), cat[:, 88:], bf, act=0)
        ctx.params = (wo, bo, wf, bf)
        ctx.save_for_backward(y, wo, wf, onset)
        ctx.set_materialize_grads(False)          # donset is None (not a zero tensor) when the onset output is unused
        return cat, onset

    @staticmethod
    def backward(ctx, dcat, donset):
        y, wo, wf, onset = ctx.saved_tensors
        bb, t, nb, _ = y.shape
        m = bb * t
        y2 = y.view(m, nb, 2)
        dcat = dcat.contiguous()
        dzo = torch.empty((m, 88), device=y.device, dtype=torch.float32)
        call('rv_sigmoid_bwd', ptr(dcat), 176, ptr(donset.contiguous()) if donset is not None else None, 88,
             ptr(onset), 88, ptr(dzo), 88, m, 88, stream())
        dzf = dcat[:, 88:]
        dy = dwo = dbo = dwf = dbf = None
        if ctx.needs_input_grad[0]:
            dy = torch.empty_like(y)
            d2 = dy.view(m, nb, 2)
            gemm(dzo, _lin_t(wo).t(), d2[..., 0])
            gemm(dzf, _lin_t(wf).t(), d2[..., 1])
        pwo, pbo, pwf, pbf = ctx.params
        if ctx.needs_input_grad[1]:
            dwo, done = _param_wgrad(dzo.t(), y2[..., 0], pwo, None, pbo)
            if not done:
                dbo = _param_bgrad(dzo, pbo)
        if ctx.needs_input_grad[3]:
            dwf, done = _param_wgrad(dzf.t(), y2[..., 1], pwf, None, pbf)
            if not done:
                dbf = _param_bgrad(dzf, pbf)
        return dy, dwo, dbo, dwf, dbf


# --------------------------------------------------------------------------------------------
# local attention
# --------------------------------------------------------------------------------------------
def _adjacent(*ts):
    """True when the tensors are contiguous and laid out back to back in memory (flat parameter / gradient buffers)."""
    for a, b in zip(ts, ts[1:]):
        if a is None or b is None or not (a.is_contiguous() and b.is_contiguous()):
            return False
        if a.data_ptr() + a.numel() * a.element_size() != b.data_ptr():
            return False
        if a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
            return False                     # neighbours by accident of the allocator, not views of one buffer
    return True


class LocalAttnFn(Function):
    """MutliHeadAttention1D.forward (model/UNet_onset.py:56-91) on x [B, L, Fin] (contiguous):
       returns (out [B, L, F], attention [B, L, G, 31]).

    The three projections write column slices [k | q | v] of ONE [B*L, 3F] buffer (the attention kernels take a row
    stride).  When W_k, W_q, W_v sit back to back in memory -- they do in FlatAdam's flat parameter buffer, in
    registration order -- the projection, its input gradient and its weight gradient are one GEMM each."""

    @staticmethod
    def forward(ctx, x, wq, wk, wv, rel, groups):
        need_gpu(x, wq)
        bb, l, fin = x.shape
        f = wq.shape[0]
        m = bb * l
        x2 = x.reshape(m, fin)
        qkv = torch.empty((m, 3 * f), device=x.device, dtype=torch.float32)
        k, q, v = qkv[:, :f], qkv[:, f:2 * f], qkv[:, 2 * f:]
        fused = _adjacent(wk, wq, wv)
        if fused:
            gemm(x2, torch.as_strided(wk, (3 * f, fin), (fin, 1)).t(), qkv)
        else:
            gemm(x2, wk.t(), k)
            gemm(x2, wq.t(), q)
            gemm(x2, wv.t(), v)
        out = torch.empty((bb, l, f), device=x.device, dtype=torch.float32)
        att = torch.empty((bb, l, groups, 31), device=x.device, dtype=torch.float32)
        call('rv_local_attn_fwd', ptr(q), ptr(k), ptr(v), 3 * f, ptr(_pack_rel(rel, f)), ptr(out), ptr(att), bb, l, groups,
             f // groups, stream())
        ctx.groups = groups
        ctx.fused = fused
        ctx.params = (wq, wk, wv, rel)
        ctx.save_for_backward(x2, wq, wk, wv, rel, qkv, att)
        ctx.mark_non_differentiable(att)
        ctx.set_materialize_grads(False)          # no zero-filled gradient tensor for the attention map
        return out, att

    @staticmethod
    def backward(ctx, dout, _datt):
        x2, wq, wk, wv, rel, qkv, att = ctx.saved_tensors
        g = ctx.groups
        bb, l = att.shape[0], att.shape[1]
        f = wq.shape[0]
        fin = x2.shape[1]
        dh = f // g
        m = bb * l
        k, q, v = qkv[:, :f], qkv[:, f:2 * f], qkv[:, 2 * f:]
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        dk, dq, dv = dqkv[:, :f], dqkv[:, f:2 * f], dqkv[:, 2 * f:]
        de = torch.empty_like(att)
        call('rv_local_attn_bwd', ptr(dout), ptr(q), ptr(k), ptr(v), 3 * f, ptr(_pack_rel(rel, f)), ptr(att), ptr(dq), ptr(dk),
             ptr(dv), 3 * f, ptr(de), bb, l, g, dh, stream())
        dx = dwq = dwk = dwv = drel = None
        fused = ctx.fused
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x2)
            if fused:
                gemm(dqkv, _lin_t(torch.as_strided(wk, (3 * f, fin), (fin, 1))).t(), dx)
            else:
                gemm(dq, _lin_t(wq).t(), dx)
                gemm(dk, _lin_t(wk).t(), dx, accumulate=True)
                gemm(dv, _lin_t(wv).t(), dx, accumulate=True)
            dx = dx.view(bb, l, -1)
        pwq, pwk, pwv, prel = ctx.params
        if ctx.needs_input_grad[1]:
            gk, gq, gv = _grad_buf(pwk), _grad_buf(pwq), _grad_buf(pwv)
            if fused and _adjacent(gk, gq, gv):
                gemm(dqkv.t(), x2, torch.as_strided(gk, (3 * f, fin), (fin, 1)), accumulate=True, deterministic=DETERMINISTIC[0], defer_ok=True)
            elif fused:
                dw3 = torch.empty((3 * f, fin), device=x2.device, dtype=torch.float32)
                gemm(dqkv.t(), x2, dw3, deterministic=DETERMINISTIC[0])
                dwk, dwq, dwv = dw3[:f], dw3[f:2 * f], dw3[2 * f:]
            else:
                sk = None
                dwq = _param_wgrad(dq.t(), x2, pwq, sk)
                dwk = _param_wgrad(dk.t(), x2, pwk, sk)
                dwv = _param_wgrad(dv.t(), x2, pwv, sk)
        if ctx.needs_input_grad[4]:
            # drel[g*dh+f, w] = sum_{b,t} q[b,t,g,f] * de[b,t,g,w]
            grel = _grad_buf(prel)
            direct = grel is not None
            drel = grel.view(f, 31) if direct else torch.zeros((f, 31), device=q.device, dtype=torch.float32)
            de2 = de.view(m, g, 31)
            # one batched split-K launch over the heads: head h reads q[:, h*dh:], de[:, h, :], writes drel[h*dh:]
            gemm(q[:, :dh].t(), de2[:, 0, :], drel[:dh], accumulate=True, deterministic=DETERMINISTIC[0], batch=g, bstrides=(dh, 31, dh * 31),
                 defer_ok=direct)       # (a zero-filled temporary handed back to autograd is filled NOW, never by a deferred launch)
            drel = None if direct else drel.view_as(rel)
        return dx, dwq, dwk, dwv, drel, None


# --------------------------------------------------------------------------------------------
# losses and VAT primitives
# --------------------------------------------------------------------------------------------
_LOSS_TICKET = os.environ.get('RV_LOSS_TICKET') == '1'


def _reduce(kind, p, t):
    need_gpu(p, t)
    n = p.numel()
    out = torch.empty((), device=p.device, dtype=torch.float32)
    ws = torch.empty((n + 2047) // 2048, device=p.device, dtype=torch.float32)
    # two launches (partials, then the fp64 fold): the single-launch form (RV_LOSS_TICKET=1: the last workgroup to arrive folds) needs
    # device-scope fences, which cost more than the second launch on this multi-XCD part (21.02 vs 21.13 ms/step in situ, round 5)
    ticket = ARENA.take(1, p.device) if _LOSS_TICKET else None
    call('rv_reduce_mean', kind, ptr(p), ptr(t), n, ptr(out), ptr(ws), ptr(ticket), stream())
    return out


class _MeanLoss(Function):
    kind = 0

    @classmethod
    def _fwd(cls, ctx, p, t):
        p = p.contiguous()
        t = t.contiguous()
        if p.shape != t.shape:
            raise ValueError(f'target size {tuple(t.shape)} must match input size {tuple(p.shape)}')
        ctx.save_for_backward(p, t)
        return _reduce(cls.kind, p, t)

    @classmethod
    def _bwd(cls, ctx, gout):
        p, t = ctx.saved_tensors
        gp = torch.empty_like(p)
        call('rv_loss_bwd', cls.kind, ptr(p), ptr(t), p.numel(), ptr(gout.contiguous()), ptr(gp), stream())
        return gp, None


class BceMeanFn(_MeanLoss):
    """F.binary_cross_entropy(p, t) (mean; soft targets allowed; log clamped at -100)."""
    kind = 0

    @staticmethod
    def forward(ctx, p, t):
        return BceMeanFn._fwd(ctx, p, t)

    @staticmethod
    def backward(ctx, gout):
        return BceMeanFn._bwd(ctx, gout)


class MseMeanFn(_MeanLoss):
    """F.mse_loss(p, t) (mean)."""
    kind = 1

    @staticmethod
    def forward(ctx, p, t):
        return MseMeanFn._fwd(ctx, p, t)

    @staticmethod
    def backward(ctx, gout):
        return MseMeanFn._bwd(ctx, gout)


def bce_mean(p, t):
    return BceMeanFn.apply(p, t.detach())


def mse_mean(p, t):
    return MseMeanFn.apply(p, t.detach())


def abs_mean(x):
    return _reduce(2, x.detach().contiguous(), None)


def l2_norm(x):
    return _reduce(3, x.detach().contiguous(), None)


class VatPerturbFn(Function):
    """x_adv = clamp(x + scale * d / ||d||_2(last dim), 0, 1) with the gradient wrt d
    (model/UNet_onset.py:130-131 through _l2_normalize :165-171)."""

    @staticmethod
    def forward(ctx, x, d, scale):
        x = x.contiguous()
        d = d.contiguous()
        n = x.shape[-1]
        rows = x.numel() // n
        x_adv = torch.empty_like(x)
        call('rv_vat_perturb_fwd', ptr(x), ptr(d), rows, n, 1.0, scale, ptr(x_adv), None, None, None, stream())
        ctx.scale = scale
        ctx.save_for_backward(x, d)
        return x_adv

    @staticmethod
    def backward(ctx, g):
        x, d = ctx.saved_tensors
        n = x.shape[-1]
        gd = torch.empty_like(d)
        call('rv_vat_perturb_bwd', ptr(g.contiguous()), ptr(x), ptr(d), x.numel() // n, n, 1.0, ctx.scale, ptr(gd),
             stream())
        return None, gd, None


def vat_adversarial(x, g, prescale, eps, nan_flag=None):
    """d = g*prescale; r_adv = eps*d/||d||; x_adv = clamp(x + r_adv, 0, 1); also returns d/||d||
    (model/UNet_onset.py:141-151,162).  No autograd."""
    x = x.contiguous()
    g = g.contiguous()
    n = x.shape[-1]
    x_adv, r_adv, dn = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    call('rv_vat_perturb_fwd', ptr(x), ptr(g), x.numel() // n, n, prescale, eps, ptr(x_adv), ptr(r_adv), ptr(dn),
         ptr(nan_flag), stream())
    return x_adv, r_adv, dn


# --------------------------------------------------------------------------------------------
# front-end
# --------------------------------------------------------------------------------------------
def melspec(audio, tables, do_log, normalise, hop=512):
    """audio [B, nsamp] -> [B, T, n_mels] (time-major) log-mel / mel power; see rv_melspec_lognorm_fwd."""
    need_gpu(audio)
    audio = audio.float()
    if audio.stride(-1) != 1:
        audio = audio.contiguous()
    bb, nsamp = audio.shape
    t = 1 + nsamp // hop
    n_mels = tables['mel_start'].numel()
    out = torch.empty((bb, t, n_mels), device=audio.device, dtype=torch.float32)
    ws = torch.empty(2 * bb, device=audio.device, dtype=torch.int32)
    call('rv_melspec_lognorm_fwd', ptr(audio), audio.stride(0), bb, nsamp, ptr(tables['window']), ptr(tables['twiddle']),
         ptr(tables['mel_start']), ptr(tables['mel_len']), ptr(tables['mel_w']), tables['mel_w'].shape[1], n_mels, hop,
         1 if do_log else 0, 1 if normalise else 0, ptr(out), t, ptr(ws), stream())
    return out


def cqtspec(audio, tables, do_log, normalise, hop=512):
    """audio [B, nsamp] -> [B, T, n_bins] (time-major) log-CQT / CQT magnitude; see rv_cqt_lognorm_fwd."""
    need_gpu(audio)
    audio = audio.float()
    if audio.stride(-1) != 1:
        audio = audio.contiguous()
    bb, nsamp = audio.shape
    t = 1 + nsamp // hop
    n_bins, kw = tables['scale'].numel(), tables['kernel_width']
    if nsamp <= kw // 2:
        raise ValueError(f'cqtspec: the signal ({nsamp} samples) must be longer than the reflect padding ({kw // 2} samples)')
    items, groups, w = tables['items'], tables['groups'], tables['w']
    out = torch.empty((bb, t, n_bins), device=audio.device, dtype=torch.float32)
    nbytes = int(_lib.load().rv_cqt_workspace_bytes(bb, nsamp, items.shape[0], hop, kw))
    ws = torch.empty((nbytes + 3) // 4, device=audio.device, dtype=torch.float32)
    call('rv_cqt_lognorm_fwd', ptr(audio), audio.stride(0), bb, nsamp, ptr(w), w.numel(), ptr(items), items.shape[0], ptr(groups),
         groups.shape[0], ptr(tables['scale']), n_bins, kw, hop, 1 if do_log else 0, 1 if normalise else 0, ptr(out), t, ptr(ws),
         nbytes, stream())
    return out


# --------------------------------------------------------------------------------------------
# Onsets&Frames baseline pieces: BiLSTM, MaxPool2d((1,2)) + Dropout, Dropout
# --------------------------------------------------------------------------------------------
_SEED = [0x1234567]


def next_seed():
    """Counter-hash seed of the next dropout draw (deterministic per process; ``seed_dropout`` resets it)."""
    _SEED[0] = (_SEED[0] * 1664525 + 1013904223) & 0xFFFFFFFF
    return _SEED[0]


def seed_dropout(seed):
    _SEED[0] = int(seed) & 0xFFFFFFFF


_DROP_EPOCH = {}


def drop_epoch(device):
    """Device-resident step counter mixed into every dropout draw: TrainStep bumps it inside the (possibly graph-captured)
    step, so replays of a captured dropout launch draw new masks."""
    key = (device.type, device.index)
    t = _DROP_EPOCH.get(key)
    if t is None:
        t = _DROP_EPOCH[key] = torch.zeros(1, dtype=torch.int64, device=device)
    return t


def bump_drop_epoch(device):
    call('rv_counter_add', ptr(drop_epoch(device)), 1, None, stream())


_LSTM_ERR = {}


def _lstm_err(device):
    key = (device.type, device.index)
    t = _LSTM_ERR.get(key)
    if t is None:
        t = _LSTM_ERR[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return t


def step_error_word(device):
    """The persistent per-device "this step is invalid" word: kernels atomicOr into it (BiLSTM time-outs), rv_adam_step skips
    the update while it is set, lstm_check() reads and clears it."""
    return _lstm_err(torch.device(device))


def lstm_check(device):
    """Raise if any BiLSTM launch since the last call gave up waiting for a neighbour workgroup (its workgroups were
    not co-resident): the results of that launch are invalid (and FlatAdam did not apply them).  Synchronises; call it at
    a point where the host waits for the step anyway (the per-step loss read-back), not per op."""
    t = _lstm_err(torch.device(device))
    if int(t.item()) != 0:
        t.zero_()
        raise RuntimeError('rv_lstm: a workgroup timed out waiting for its neighbours (launch not co-resident); '
                           'the BiLSTM outputs of this step are invalid')


class BiLstmFn(Function):
    """nn.LSTM(I, H, batch_first=True, bidirectional=True)(x)[0] with zero initial state
    (model/onset_frame_VAT.py:614; Onset_Stack.forward_LSTM :370-381, Combine_Stack.forward_LSTM :401-410).
    Parameter order: forward direction (w_ih [4H,I], w_hh [4H,H], b_ih, b_hh) then the ``_reverse`` four."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r):
        need_gpu(x, w_ih)
        bb, t, i = x.shape
        h = w_hh.shape[1]
        x2 = x.reshape(bb * t, i)
        xg = torch.empty((bb * t, 2, 4 * h), device=x.device, dtype=torch.float32)
        gemm(x2, w_ih.t(), xg[:, 0, :], b_ih + b_hh)
        gemm(x2, w_ih_r.t(), xg[:, 1, :], b_ih_r + b_hh_r)
        out = torch.empty((bb, t, 2 * h), device=x.device, dtype=torch.float32)
        train = any(ctx.needs_input_grad)
        gates = torch.empty((bb, t, 2, 4, h), device=x.device, dtype=torch.float32) if train else None
        cs = torch.empty((bb, t, 2, h), device=x.device, dtype=torch.float32) if train else None
        flags = torch.empty(_lib.load().rv_lstm_flag_bytes(h) // 4, device=x.device, dtype=torch.int32)
        w_hh, w_hh_r = w_hh.contiguous(), w_hh_r.contiguous()
        # a time-out is atomicOr'ed by the kernel itself into the persistent per-device word (ops.lstm_check / FlatAdam skip)
        call('rv_lstm_fwd', ptr(xg), ptr(w_hh), ptr(w_hh_r), ptr(out), ptr(gates), ptr(cs), ptr(flags), ptr(_lstm_err(x.device)),
             bb, t, h, stream())
        ctx.params = (w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r)
        ctx.save_for_backward(x2, out, gates, cs, w_ih, w_hh, w_ih_r, w_hh_r)
        ctx.dims = (bb, t, i, h)
        ctx.flags = flags
        return out

    @staticmethod
    def backward(ctx, dout):
        x2, out, gates, cs, w_ih, w_hh, w_ih_r, w_hh_r = ctx.saved_tensors
        bb, t, i, h = ctx.dims
        dout = dout.contiguous()
        dxg = torch.empty((bb * t, 2, 4 * h), device=dout.device, dtype=torch.float32)
        call('rv_lstm_bwd', ptr(dout), ptr(w_hh), ptr(w_hh_r), ptr(gates), ptr(cs), ptr(dxg), ptr(ctx.flags),
             ptr(_lstm_err(dout.device)), bb, t, h, stream())
        # h_{prev} of every step: the output shifted by one step along each direction's own time arrow
        hprev = torch.zeros((bb, t, 2, h), device=dout.device, dtype=torch.float32)
        o4 = out.view(bb, t, 2, h)
        hprev[:, 1:, 0] = o4[:, :-1, 0]
        hprev[:, :-1, 1] = o4[:, 1:, 1]
        hprev = hprev.view(bb * t, 2, h)
        grads = [None] * 9
        if ctx.needs_input_grad[0]:
            dx = torch.empty((bb * t, i), device=dout.device, dtype=torch.float32)
            gemm(dxg[:, 0, :], w_ih, dx)
            gemm(dxg[:, 1, :], w_ih_r, dx, accumulate=True)
            grads[0] = dx.view(bb, t, i)
        for d, base in ((0, 1), (1, 5)):
            dz = dxg[:, d, :]
            p_ih, p_hh, p_bi, p_bh = ctx.params[base - 1:base + 3]
            ih_bias = hh_bias = False
            if ctx.needs_input_grad[base]:
                if ctx.needs_input_grad[base + 2]:
                    grads[base], ih_bias = _param_wgrad(dz.t(), x2, p_ih, None, p_bi)
                else:
                    grads[base] = _param_wgrad(dz.t(), x2, p_ih, None)
            if ctx.needs_input_grad[base + 1]:
                if ctx.needs_input_grad[base + 3]:
                    grads[base + 1], hh_bias = _param_wgrad(dz.t(), hprev[:, d, :], p_hh, None, p_bh)
                else:
                    grads[base + 1] = _param_wgrad(dz.t(), hprev[:, d, :], p_hh, None)
            if ctx.needs_input_grad[base + 2] and not ih_bias:
                grads[base + 2] = _param_bgrad(dz, p_bi)
            if ctx.needs_input_grad[base + 3] and not hh_bias:
                grads[base + 3] = _param_bgrad(dz, p_bh)
        return tuple(grads)


class PoolDropFn(Function):
    """nn.MaxPool2d((1,2)) then nn.Dropout(p) on an NHWC tensor (model/onset_frame_VAT.py:336-343)."""

    @staticmethod
    def forward(ctx, x, p, training):
        need_gpu(x)
        x = x.contiguous()
        bb, hh, w, c = x.shape
        y = torch.empty((bb, hh, w // 2, c), device=x.device, dtype=torch.float32)
        code = torch.empty((bb, hh, w // 2, c), device=x.device, dtype=torch.uint8)
        p = float(p) if training else 0.0
        call('rv_maxpool_w2_dropout_fwd', ptr(x), ptr(y), ptr(code), bb * hh, w, c, p, next_seed(), ptr(drop_epoch(x.device)), stream())
        ctx.p, ctx.xshape = p, tuple(x.shape)
        ctx.save_for_backward(code)
        return y

    @staticmethod
    def backward(ctx, dy):
        code, = ctx.saved_tensors
        bb, hh, w, c = ctx.xshape
        dx = torch.empty(ctx.xshape, device=dy.device, dtype=torch.float32)
        call('rv_maxpool_w2_dropout_bwd', ptr(dy.contiguous()), ptr(code), ptr(dx), bb * hh, w, c, ctx.p, stream())
        return dx, None, None


class DropoutFn(Function):
    """nn.Dropout(p) in training mode (model/onset_frame_VAT.py:346-348)."""

    @staticmethod
    def forward(ctx, x, p):
        need_gpu(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        code = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
        call('rv_dropout', ptr(x), ptr(y), ptr(code), None, x.numel(), float(p), next_seed(), ptr(drop_epoch(x.device)), stream())
        ctx.p = float(p)
        ctx.save_for_backward(code)
        return y

    @staticmethod
    def backward(ctx, dy):
        code, = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        call('rv_dropout', ptr(dy), ptr(dx), None, ptr(code), dy.numel(), ctx.p, 0, None, stream())
        return dx, None


def dropout(x, p, training):
    return DropoutFn.apply(x, p) if (training and p > 0.0) else x


# --------------------------------------------------------------------------------------------
# Thickstun baseline (csrc/thickstun.hip): window-sharing form of model/Thickstun_model.py
# --------------------------------------------------------------------------------------------
THICK_F = 51               # rows of CNN_freq's output: (229 - 128) / 2 + 1
THICK_TAPS = 25
THICK_LINEAR_SPLITK = 48   # fixed (not tuned per M): a frame's logits must not depend on how many frames share the launch (chunked evaluation)


def thick_wj(w):
    """CNN_time.weight [N, C, 1, 25] -> wj [25][N][C] (tap-major: the forward kernel's and the input-gradient GEMMs' operand)."""
    n, c, _, taps = w.shape
    return _pack_plain(w, ('thick', 'wj'), (taps, n, c, c * taps, taps, 0, 0, 1), w.numel()).view(taps, n, c)


def thick_feature_index(c, f, channels=4096, rows=THICK_F):
    """(checkpoint feature index c*rows + f of linear.weight, z3 feature index f*channels + c) of channel c, frequency row f."""
    return c * rows + f, f * channels + c


def thick_wlt(w, channels):
    """linear.weight [88, channels*51] in the checkpoint's c*51 + f feature order -> [51*channels, 88]: transposed, z3's f*channels + c order."""
    n, k = w.shape
    rows = k // channels
    return _pack_plain(w, ('thick', 'wlt'), (rows, channels, n, rows, k, 0, 0, 1), w.numel()).view(k, n)


def thick_wlt_grad_to_checkpoint(dwlt, channels):
    """Gradient in thick_wlt's layout [51*channels, 88] -> linear.weight's [88, channels*51]."""
    k, n = dwlt.shape
    return dwlt.view(k // channels, channels, n).permute(2, 1, 0).reshape(n, k)


class ThickFreqFn(Function):
    """z2 = relu(CNN_freq) per frame: x [B, Tin, 229] time-major -> [B, 51, Tin + 2*pad, 128]; the 2*pad zero frames of the reference's
    F.pad come out as relu(bias).  No gradient flows to x (the spectrogram is a leaf)."""

    @staticmethod
    def forward(ctx, x, w, b, pad):
        need_gpu(x, w, b)
        x = x.contiguous()
        bb, tin, bins = x.shape
        assert bins == 229 and tuple(w.shape) == (128, 1, 128, 1), (x.shape, w.shape)
        z2 = torch.empty((bb, THICK_F, tin + 2 * pad, 128), device=x.device, dtype=torch.float32)
        call('rv_thick_freq_fwd', ptr(x), ptr(w), ptr(b), ptr(z2), bb, tin, pad, stream())
        ctx.pad = pad
        ctx.save_for_backward(x, z2)
        return z2

    @staticmethod
    def backward(ctx, dz2):
        x, z2 = ctx.saved_tensors
        dz2 = dz2.contiguous()
        bb, tin, _ = x.shape
        dw = torch.empty((128, 1, 128, 1), device=x.device, dtype=torch.float32)
        db = torch.empty(128, device=x.device, dtype=torch.float32)
        nbytes = _lib.load().rv_thick_freq_bwd_workspace_bytes(bb, tin, ctx.pad)
        ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32)
        call('rv_thick_freq_bwd', ptr(dz2), ptr(z2), ptr(x), ptr(dw), ptr(db), bb, tin, ctx.pad, 0, ptr(ws), nbytes, stream())
        return None, dw, db, None


class ThickTconvFn(Function):
    """z3 = relu(CNN_time) over the Hankel view of z2 [B, 51, T+24, 128] -> [B, T, 51, N].  Forward: rv_thick_tconv_fwd (A operand
    stationary in LDS).  Backward on rv_gemm through strided views: the input gradient as 25 accumulating GEMMs per clip (one per tap,
    the 51 frequency rows batched), the weight gradient as one accumulating GEMM per (clip, frequency row) with the bias gradient riding
    along as the row sums -- plain read-modify-write in stream order, no atomics, so both are run-to-run reproducible.
    The incoming dz3 is expected to carry z3's ReLU mask already (ThickLinearFn applies it in its epilogue)."""

    @staticmethod
    def forward(ctx, z2, w, b):
        need_gpu(z2, w, b)
        bb, rows, tp, c = z2.shape
        n = w.shape[0]
        t = tp - (THICK_TAPS - 1)
        assert rows == THICK_F and c == 128 and tuple(w.shape[1:]) == (c, 1, THICK_TAPS) and t >= 1, (z2.shape, w.shape)
        z3 = torch.empty((bb, t, rows, n), device=z2.device, dtype=torch.float32)
        call('rv_thick_tconv_fwd', ptr(z2), ptr(thick_wj(w)), ptr(b), ptr(z3), bb, t, n, stream())
        ctx.save_for_backward(z2, w)
        return z3

    @staticmethod
    def backward(ctx, dz3):
        z2, w = ctx.saved_tensors
        dz3 = dz3.contiguous()
        bb, rows, tp, c = z2.shape
        n = w.shape[0]
        t = tp - (THICK_TAPS - 1)
        dz2 = dw = db = None
        if ctx.needs_input_grad[0]:
            dz2 = thick_tconv_dgrad(dz3, thick_wj(w), bb, t)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dwflat, db = thick_tconv_wgrad(dz3, z2)
            dw = dwflat.view(n, THICK_TAPS, c).permute(0, 2, 1).reshape(n, c, 1, THICK_TAPS)      # [n][j][c] -> the checkpoint's [n][c][1][j]
        return dz2, dw, db


def thick_tconv_dgrad(dz3, wj, bb, t):
    """dz2[b,f,s,c] = sum_j sum_n dz3[b,s-j,f,n] * W[n,c,j] (without z2's ReLU mask: its consumer applies it on load)."""
    taps, n, c = wj.shape
    rows, tp = THICK_F, t + taps - 1
    dz2 = torch.zeros((bb, rows, tp, c), device=dz3.device, dtype=torch.float32)
    for b in range(bb):
        a = dz3.as_strided((t, n), (rows * n, 1), dz3.storage_offset() + b * t * rows * n)
        for j in range(taps):
            out = dz2.as_strided((t, c), (c, 1), (b * rows * tp + j) * c)
            gemm(a, wj[j], out, accumulate=True, splitk=1, batch=rows, bstrides=(n, 0, tp * c))
    return dz2


def thick_tconv_wgrad(dz3, z2):
    """(dW [N, 25*128] in (tap, channel) order, dbias [N]):  dW[n, j*128+c] = sum_{b,f,t} dz3[b,t,f,n] * z2[b,f,t+j,c]."""
    bb, t, rows, n = dz3.shape
    tp, c = z2.shape[2], z2.shape[3]
    k = (tp - t + 1) * c
    dw = torch.zeros((n, k), device=dz3.device, dtype=torch.float32)
    db = torch.zeros(n, device=dz3.device, dtype=torch.float32)
    for b in range(bb):
        for f in range(rows):
            a = dz3.as_strided((n, t), (1, rows * n), dz3.storage_offset() + (b * t * rows + f) * n)
            hankel = z2.as_strided((t, k), (c, 1), z2.storage_offset() + (b * rows + f) * tp * c)
            gemm(a, hankel, dw, accumulate=True, splitk=1, a_rowsum=db)
    return dw, db


class ThickLinearFn(Function):
    """p = sigmoid(z3 @ W^T) for z3 [M, K] >= 0 (the reference's torch.relu(torch.flatten(z3)) is the identity on it) and the checkpoint's
    linear.weight [88, K] (c*51 + f feature order; read through thick_wlt).  Backward returns the gradient of z3's PRE-activation:
    rv_thick_linear_dz applies z3's ReLU mask in its epilogue, so no separate pass over the 535 MB gradient exists."""

    @staticmethod
    def forward(ctx, z3, w, channels):
        need_gpu(z3, w)
        m, k = z3.shape
        n = w.shape[0]
        assert z3.is_contiguous() and tuple(w.shape) == (n, k)
        wlt = thick_wlt(w, channels)
        y = torch.empty((m, n), device=z3.device, dtype=torch.float32)
        gemm(z3, wlt, y, None, 1, splitk=THICK_LINEAR_SPLITK)
        ctx.channels = channels
        ctx.save_for_backward(z3, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        z3, w, y = ctx.saved_tensors
        dy = dy.contiguous()
        m, k = z3.shape
        n = w.shape[0]
        wlt = thick_wlt(w, ctx.channels)
        dz = torch.empty_like(dy)
        call('rv_sigmoid_bwd', ptr(dy), n, None, 0, ptr(y), n, ptr(dz), n, m, n, stream())
        dz3 = dw = None
        if ctx.needs_input_grad[0]:
            dz3 = torch.empty_like(z3)
            call('rv_thick_linear_dz', ptr(dz), ptr(wlt), ptr(z3), ptr(dz3), m, k, n, stream())
        if ctx.needs_input_grad[1]:
            dwlt = torch.empty((k, n), device=z3.device, dtype=torch.float32)
            gemm(z3.t(), dz, dwlt, splitk=1)
            dw = thick_wlt_grad_to_checkpoint(dwlt, ctx.channels)
        return dz3, dw, None


# ---- note velocities (csrc/velocity.hip; the definition is reconvat_amd/velocity.py) -------------------------------------
VELOCITY_PARAMS = 1121


def _f32_dev(t):
    """float32, contiguous and 4-byte aligned on its device, as the velocity kernels read their buffers."""
    return t.detach().to(torch.float32).contiguous()


def _velocity_args(spec, table, params):
    import numpy as np
    need_gpu(spec, params)
    if spec.dim() != 3:
        raise ValueError(f'expected a [B, T, n_bins] spectrogram, got {tuple(spec.shape)}')
    tab = np.ascontiguousarray(np.asarray(table, dtype=np.int32))
    if tab.shape != (88, 8):
        raise ValueError(f'expected an [88, 8] bin table, got {tab.shape}')
    params = _f32_dev(params).reshape(-1)
    if params.numel() != VELOCITY_PARAMS:
        raise ValueError(f'expected {VELOCITY_PARAMS} packed parameters, got {params.numel()}')
    return _f32_dev(spec), tab, params


def velocity_roll(spec, table, params):
    """v^ [B, T, 88] of a normalised spectrogram [B, T, n_bins] (rv_velocity_roll); `table`: velocity.harmonic_bins (host, int32
    [88, 8]); `params`: the 1121 packed parameters."""
    spec, tab, params = _velocity_args(spec, table, params)
    b, t, n_bins = spec.shape
    out = torch.empty((b, t, 88), dtype=torch.float32, device=spec.device)
    with torch.cuda.device(spec.device):
        call('rv_velocity_roll', ptr(spec), spec.numel(), b, t, n_bins, tab.ctypes.data, ptr(params), params.numel(), ptr(out),
             out.numel(), stream())
    return out


def velocity_loss_grad(spec, table, params, target, mask):
    """(loss [], gradient [1121]) on the device: rv_velocity_loss_grad, two launches, the same bits on every run."""
    spec, tab, params = _velocity_args(spec, table, params)
    need_gpu(target, mask)
    b, t, n_bins = spec.shape
    target, mask = _f32_dev(target), _f32_dev(mask)
    if tuple(target.shape) != (b, t, 88) or target.shape != mask.shape:
        raise ValueError(f'expected target and mask of shape {(b, t, 88)}, got {tuple(target.shape)} and {tuple(mask.shape)}')
    with torch.cuda.device(spec.device):
        ws_bytes = _lib.load().rv_velocity_workspace_bytes(b, t)
        ws = torch.empty(max(ws_bytes, 16) // 4, dtype=torch.float32, device=spec.device)
        loss = torch.empty((), dtype=torch.float32, device=spec.device)
        grad = torch.empty(VELOCITY_PARAMS, dtype=torch.float32, device=spec.device)
        call('rv_velocity_loss_grad', ptr(spec), spec.numel(), b, t, n_bins, tab.ctypes.data, ptr(params), params.numel(), ptr(target),
             ptr(mask), target.numel(), ptr(loss), ptr(grad), grad.numel(), ptr(ws), ws_bytes, stream())
    return loss, grad


class VelocityLossFn(Function):
    """sum m (v^ - target)^2 / sum m as a function of the packed parameters; the gradient is computed with the loss and scaled by
    grad_output in backward.  The spectrogram gets none: the front end is fixed."""

    @staticmethod
    def forward(ctx, params, spec, table, target, mask):
        loss, grad = velocity_loss_grad(spec, table, params, target, mask)
        ctx.save_for_backward(grad)
        ctx.shape = params.shape
        return loss

    @staticmethod
    def backward(ctx, gout):
        grad, = ctx.saved_tensors
        return (grad * gout).reshape(ctx.shape), None, None, None, None


def velocity_loss(spec, table, params, target, mask):
    return VelocityLossFn.apply(params, spec.detach(), table, target.detach(), mask.detach())
