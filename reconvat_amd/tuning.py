"""Kernel selection: which tile a conv launch, which partition a weight gradient, which split-K factor a GEMM runs.  Pure host logic over the plan
table (plans.py) and injected launch / timing callables -- importable and testable without a GPU; `best_of_bursts` alone touches torch.cuda.  The
mode (ops.AUTOTUNE: 'table' | True | False) is an argument everywhere: this module does not import ops."""
import operator
import os
import sys

from . import plans

# The algo code of rv_conv_fwd: TH << 12 | family << 8 | NT << 4 | MT (+ ALGO_BF16); 0 = library default, 1 / 2 = the direct / the LDS kernel with the
# library's own tile.  The authoritative description is next to conv_fwd_impl in csrc/conv.hip; this table is its host-side mirror.
ALGO_BF16 = 1 << 20       # bf16 operands (the library ignores the bit outside the persistent 3x3 kernel / 16-channel chunks)
# family -> (kernel, waves per workgroup, Winograd tile (fp32 only: no bf16 form), K-split direct tile)
FAMILIES = {
    1: ('conv_mfma_k', 4, False, False),         # direct (LDS-free) kernel with a forced NT x MT register tile, every mode
    2: ('conv3x3_lds_k', 4, False, False),       # persistent LDS/DMA-pipelined 3x3 kernel; TH = rows per band (0: as many as the tile slots hold)
    3: ('conv3x3_lds_k', 8, False, False),
    4: ('conv3x3_lds_k', 16, False, False),
    5: ('conv_mfma_k', 4, False, True),          # direct kernel, K loop split over the four waves (1x1 / 2x2 modes, deep layers)
    6: ('conv3x3_wino_k', 8, True, False),       # Winograd F(2x2,3x3), cin % 16 == 0, bands of an even number of rows
    7: ('conv3x3_lds_k', 12, False, False),      # MT 3 / 5 / 6: the band sizes that fit whole 57 / 114 / 229-pixel rows
    8: ('conv3x3_wino2_k', 8, True, False),      # software-pipelined Winograd (conv_wino2.hip), full-chunk patch
    9: ('conv3x3_wino2_k', 8, True, False),      # ... half-chunk patch
    10: ('conv3x3_wino_k', 8, True, False),      # patch read half a chunk at a time (the only form with NT = 2)
    11: ('conv3x3_wino2_k', 4, True, False),
    12: ('conv3x3_wino_k', 12, True, False),     # half-chunk patch
    13: ('conv3x3_wino2_k', 12, True, False),    # half-chunk patch
    14: ('conv3x3_wino_k', 4, True, False),      # half-CU experiment: forced only, never a tuner candidate or a table entry
}
WINOGRAD_FAMILIES = tuple(f for f, v in FAMILIES.items() if v[2])       # a bf16 launch of such a shape runs the library-default direct tile instead
KSPLIT_FAMILIES = tuple(f for f, v in FAMILIES.items() if v[3])
LDS_WAVES = {f: v[1] for f, v in FAMILIES.items() if v[0] == 'conv3x3_lds_k'}

_algo_cache = {}           # conv launch key (+ ('bf16',)) -> algo
_algo_unchecked = set()    # table entries borrowed from another batch size: legality is checked by their first launch
_tune_us = {}              # ('conv' | 'wgrad' | 'gemm', key) -> microseconds the on-line tuner measured for its choice
_tune_top = {}             # (what, key) -> [(us, choice)] the three fastest candidates (tools/tune_plans.py --in-situ re-ranks near ties in the step)
_gemm_splitk = {}          # (M, N, K, batch, A k-fast, B k-fast, act, accumulate) -> split-K factor in use
_wgrad_tuned = set()       # (taps, B, Hv, Wv, Ca, Cb): shapes whose partition this process has decided
_wgrad_plans = {}          # (taps, B, Hv, Wv, Ca, Cb) -> (nw, wgs): what this process pinned in the library (tools/tune_plans.py dumps it)
# The library keys its partition by (taps, B, Hv, Ca, Cb), without the row width Wv: shapes that differ only in width -- the same layer of a
# 229-bin and of a 176-bin model -- share ONE library entry.  _wgrad_owner records which full shape last pinned each entry; a launch of another
# width re-pins the entry to its own plan (or the library default) first, so no shape runs the partition decided for another width.
_wgrad_owner = {}          # (taps, B, Hv, Ca, Cb) -> (taps, B, Hv, Wv, Ca, Cb)


def encode(fam, nt, mt, th=0):
    return th << 12 | fam << 8 | nt << 4 | mt


def decode(algo):
    """(family, NT, MT, rows per band, bf16) of an algo code."""
    return (algo >> 8) & 15, (algo >> 4) & 15, algo & 15, (algo >> 12) & 255, bool(algo & ALGO_BF16)


def bf16_form(algo):
    """What the bf16-operand launch of a shape whose fp32 choice is `algo` runs: the library-default direct tile for a Winograd one."""
    if decode(algo)[0] in WINOGRAD_FAMILIES:
        algo = 0
    return algo if algo == 1 or decode(algo)[0] == 1 else algo | ALGO_BF16


# (Winograd family, the (NT, MT) tiles the tuner offers, pipelined form: the taller half of the legal band heights only -- short bands lose to their halo)
_WINOGRAD_TILES = ((6, ((1, 1),), False), (10, ((1, 1), (2, 1)), False), (12, ((1, 1),), False),
                   (8, ((1, 1),), True), (9, ((1, 1), (2, 1), (1, 2)), True), (11, ((1, 2), (2, 1)), True), (13, ((1, 1),), True))


def conv_candidates(mode, h, w, cin, cout, *, winograd=True, wino2=True, families=None):
    """The tiles the on-line tuner times for one conv shape, in the order it times them (the first strictly faster one wins, so order decides ties)."""
    ntile_n = (4 * cout if mode == 3 else cout + 15) // 16
    cands = [1, 2] if mode == 0 else [0]
    for nt in (1, 2, 3, 4):
        if ntile_n % nt:
            continue
        cands += [encode(1, nt, mt) for mt in (1, 2, 4)]
        if mode != 0:
            cands += [encode(5, nt, mt) for mt in (1, 2, 4) if nt * mt <= 4]
        else:
            for fam, mts in ((2, (1, 2, 4, 8)), (3, (1, 2, 4)), (4, (1, 2, 4)), (7, (1, 2, 3, 4, 5, 6))):     # 12 waves: 3 .. 18 tiles per SIMD and band
                cands += [encode(fam, nt, mt) for mt in mts]
    if mode != 0:
        return cands
    # rows per band: the tile slots of a (waves, MTW) pair hold th_max rows; fewer rows trade padding for a band count that divides over the
    # 256 workgroup slots (the deep layers have only a few bands per image)
    extra = []
    for cand in cands:
        fam, _, mt, _, _ = decode(cand)
        th_max = min(h, mt * 16 * LDS_WAVES[fam] // w) if fam in LDS_WAVES else 0
        if th_max < 2:
            continue
        nb0 = -(-h // th_max)
        for nb in range(nb0, nb0 + 4):
            th = -(-h // nb)
            if 0 < th < th_max and th < 256:
                extra.append(th << 12 | cand)
    cands += sorted(set(extra))
    if cin % 16 == 0 and winograd:
        wt = (w + 1) // 2
        for fam, tiles, pipelined in _WINOGRAD_TILES:
            for nt, mt in tiles if (wino2 or not pipelined) else ():
                if ntile_n % nt == 0:
                    # bands of an even number of rows: 0 (as many as the tile slots hold), then the heights that change the band count
                    th_max = min(h, 2 * ((FAMILIES[fam][1] * mt * 16) // wt))
                    ths = [t for t in range(2, th_max, 2) if -(-h // t) != -(-h // (t + 2)) and (t >= th_max // 2 or not pipelined)]
                    cands += [encode(fam, nt, mt, t) for t in [0] + ths]
    if families:                                  # experiment: restrict the tile families the tuner may pick (1 / 2 also name the codes 1 / 2)
        cands = [c for c in cands if decode(c)[0] in families or (c in (1, 2) and c in families)]
    return cands


def wgrad_candidates(taps, hv, *, winograd=True):
    """(waves per workgroup, workgroups) partitions of the MFMA weight-gradient kernel; nw = 24: eight waves, Winograd F(3x3, 2x2) form (wgrad_wino_k)."""
    cands = [(8, 256), (8, 512), (4, 256), (4, 512), (8, 128), (8, 1024)]
    if taps == 9 and hv % 2 == 0 and winograd:
        cands += [(24, 256), (24, 512), (24, 128)]
    return cands


def gemm_splitk_candidates(m, n, k, cands):
    blocks = ((m + 63) // 64) * ((n + 63) // 64)
    return [s for s in cands if s == 1 or not (k // s < 64 or blocks * s > 4096)]


def best_of_bursts(launch, stream, bursts=2, reps=3):
    """Milliseconds per launch: the best of `bursts` bursts of `reps` launches (HIP events on the launch stream; less timing noise than one burst)."""
    import torch
    times = []
    for _ in range(bursts):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            launch()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return min(times) / reps


def faster_by_3_percent(t, best):
    """Split-K factors are tried in rising order: a larger factor must win by 3 %, ties go to fewer slices."""
    return t < 0.97 * best


def pick(cands, try_launch, time_of, better=operator.lt, default=0):
    """(choice, its time, the three fastest as sorted [(time, candidate)]): candidates whose trial launch returns non-zero do not fit the shape and are
    skipped; of the rest the first one no later one is `better` than wins.  No legal candidate: (default, None, [])."""
    best, choice, ranked = None, default, []
    for cand in cands:
        if try_launch(cand) != 0:
            continue
        t = time_of(cand)
        ranked.append((t, cand))
        if best is None or better(t, best):
            best, choice = t, cand
    return choice, best, sorted(ranked)[:3]


def tune(what, key, cands, try_launch, time_of, better=operator.lt, default=0, describe=str):
    """On-line choice for one shape (time_of in milliseconds): pick(), recorded in _tune_us / _tune_top."""
    choice, best, ranked = pick(cands, try_launch, time_of, better, default)
    if best is not None:
        _tune_us[(what, key)] = best * 1e3
        _tune_top[(what, key)] = [(t * 1e3, c) for t, c in ranked]
        if os.environ.get('RV_TUNE_LOG'):
            print(f'[tune] {what} {describe(choice)} {best * 1e3:.1f} us', file=sys.stderr)
    return choice


def choose_conv(mode, base_key, bf16=False, forced=None, online=None, first_launch=None):
    """The algo code for a launch of the conv shape base_key = (conv mode, B, H, W, cin, cout, ild, old, stats, bnbwd) in the tuning mode `mode`.  In this order: a
    forced code; the per-shape cache; the plan table (an entry borrowed from another batch size is marked unchecked); the on-line tuner `online(key)` (None under
    hipGraph capture: library default, not cached); the legality check of an unchecked entry, which IS its first launch (`first_launch(algo)` -> status; a tile that
    does not fit this batch size becomes the library default); the bf16 form.  Returns None when first_launch has already run the conv."""
    conv_mode, _, _, _, cin, cout = base_key[:6]
    algo, key = forced or 0, None
    if forced is None and mode and cin % 8 == 0 and (cout > 2 or conv_mode == 3):     # (the small-channel VALU kernels have one form)
        # the bf16-operand variant of a shape is its own cache entry in every mode: its tile may differ from the fp32 one (the fp32
        # Winograd tiles have no bf16 form), and a bf16 launch must never overwrite what the fp32 launches of the same shape run
        key = base_key + ('bf16',) if bf16 else base_key
        algo = _algo_cache.get(key, -1)
        if algo < 0 and mode == 'table':
            hit = plans.lookup_conv(base_key)
            algo = hit[0] if hit is not None else 0
            if bf16 and decode(algo)[0] in WINOGRAD_FAMILIES:
                algo = 0
            _algo_cache[key] = algo
            if hit is not None and not hit[1] and algo != 0:
                _algo_unchecked.add(key)
        if algo < 0:
            tuned = online(key) if online is not None else None
            algo = 0 if tuned is None else _algo_cache.setdefault(key, tuned)
    if key in _algo_unchecked:
        _algo_unchecked.discard(key)
        if first_launch(bf16_form(algo) if bf16 else algo) == 0:
            return None
        algo = _algo_cache[key] = 0
    return bf16_form(algo) if bf16 else algo


def _pin_wgrad(lib, full, plan):
    """Pin `plan` ((nw, wgs); None = library default) for the full shape `full` and record it as the owner of its library entry."""
    taps, bb, hv, _, ca, cb = full
    if lib.rv_conv_wgrad_set_plan(taps, bb, hv, ca, cb, *(plan if plan is not None else (0, 0))) != 0:
        return False
    _wgrad_owner[(taps, bb, hv, ca, cb)] = full
    return True


def _repin_wgrad(lib, full):
    """Before a launch of the shape `full`: if another width pinned the shared library entry since, restore this shape's plan.
    Host-only (legal under hipGraph capture); a no-op while one width uses the entry, i.e. for every launch of a single model."""
    taps, bb, hv, _, ca, cb = full
    owner = _wgrad_owner.get((taps, bb, hv, ca, cb))
    if owner is not None and owner != full:
        _pin_wgrad(lib, full, _wgrad_plans.get(full))


def wgrad_plan_for(lib, key, mode, fallback_key=None):
    """Before a launch of the shape `key`, host-only (legal under hipGraph capture).  First time: pin the table's entry (or the nearest batch's) in table mode,
    else what this process decided for `fallback_key` (a merged launch of n passes: the plan tuned for one pass).  Afterwards: re-pin only."""
    if key in _wgrad_tuned:
        return _repin_wgrad(lib, key)
    _wgrad_tuned.add(key)
    plan = (plans.lookup_wgrad(key) if mode == 'table' else None) or _wgrad_plans.get(fallback_key)
    if plan is not None and _pin_wgrad(lib, key, tuple(plan)):
        _wgrad_plans[key] = tuple(plan)
    else:
        _repin_wgrad(lib, key)
