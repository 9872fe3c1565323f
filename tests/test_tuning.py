"""Kernel selection (reconvat_amd/tuning.py) on the CPU: the candidate lists the on-line tuner times (recorded from the enumeration that used to sit
inside ops._conv_call, tests/golden/tuner_candidates.json), the algo code, the tie rules with made-up times, the table-mode choice with a recording
stand-in for the launch, and the pageable path of the host table behind the deferred launches."""
import json
import os

import pytest
import torch

from reconvat_amd import ops, plans, tuning

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'tuner_candidates.json')) as fh:
    GOLDEN = json.load(fh)


def _knobs(rec):
    kn = dict(rec['knobs'])
    if 'families' in kn:
        kn['families'] = set(kn['families'])
    return kn


def test_conv_candidates_are_the_recorded_lists_in_order():
    counts = {}
    for rec in GOLDEN['conv']:
        got = tuning.conv_candidates(*rec['shape'], **_knobs(rec))
        assert got == rec['cands'], (rec['shape'], rec['knobs'])
        assert len(set(got)) == len(got)
        if not rec['knobs']:
            counts[tuple(rec['shape'])] = len(got)
    want = {(0, 640, 229, 16, 16): 30, (0, 160, 57, 64, 64): 151, (0, 640, 229, 8, 16): 21, (1, 640, 229, 16, 16): 7, (2, 640, 229, 16, 32): 12,
            (3, 160, 57, 64, 32): 16, (0, 40, 14, 256, 256): 267}
    assert {k: counts[k] for k in want} == want
    first = tuning.conv_candidates(0, 640, 229, 16, 16)
    assert first[:3] == [0x1, 0x2, 0x111] and first[-1] == 0xd11
    assert tuning.conv_candidates(0, 40, 14, 256, 256)[-1] == 0x26d11
    assert {frozenset(rec['knobs']) for rec in GOLDEN['conv']} >= {frozenset(), frozenset({'winograd'}), frozenset({'wino2'}), frozenset({'families'})}


def test_wgrad_candidates_are_the_recorded_lists_in_order():
    for rec in GOLDEN['wgrad']:
        assert tuning.wgrad_candidates(rec['taps'], rec['hv'], **rec['knobs']) == [tuple(c) for c in rec['cands']], rec
    assert {(r['taps'], r['hv'] % 2) for r in GOLDEN['wgrad']} >= {(9, 0), (9, 1), (4, 0)}


def test_gemm_splitk_candidates_filter():
    all_ = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)
    assert tuning.gemm_splitk_candidates(64, 64, 5120, all_) == list(all_)
    assert tuning.gemm_splitk_candidates(64, 64, 512, all_) == [1, 2, 3, 4, 6, 8]              # k // s >= 64
    assert tuning.gemm_splitk_candidates(64 * 32, 64 * 32, 1 << 20, all_) == [1, 2, 3, 4]       # blocks * s <= 4096
    assert tuning.gemm_splitk_candidates(64, 64, 8, (1,)) == [1]


def test_algo_code_round_trips_and_matches_the_hand_written_shifts():
    codes = {c for rec in GOLDEN['conv'] for c in rec['cands']} | set(plans.conv_entries().values())
    codes |= {tuning.encode(f, nt, mt, th) for f in tuning.FAMILIES for nt in (1, 4) for mt in (1, 8) for th in (0, 255)}
    for algo in codes:
        fam, nt, mt, th, bf16 = tuning.decode(algo)
        assert (fam, nt, mt, th, bf16) == ((algo >> 8) & 15, (algo >> 4) & 15, algo & 15, algo >> 12, False), hex(algo)
        assert tuning.encode(fam, nt, mt, th) == algo
        assert tuning.decode(algo | tuning.ALGO_BF16) == (fam, nt, mt, th, True)
        assert fam == 0 and algo in (0, 1, 2) or fam in tuning.FAMILIES, hex(algo)
    assert tuning.WINOGRAD_FAMILIES == (6, 8, 9, 10, 11, 12, 13, 14) and tuning.LDS_WAVES == {2: 4, 3: 8, 4: 16, 7: 12}
    assert tuning.KSPLIT_FAMILIES == (5,)
    assert ops.WINOGRAD_FAMILIES is tuning.WINOGRAD_FAMILIES and ops.ALGO_BF16 == tuning.ALGO_BF16 == 1 << 20
    for name in ('_algo_cache', '_tune_us', '_tune_top', '_wgrad_plans', '_wgrad_tuned', '_gemm_splitk'):
        assert getattr(ops, name) is getattr(tuning, name), name


def _pick(times, illegal=(), **kw):
    timed = []

    def time_of(c):
        timed.append(c)
        return times[c]
    return tuning.pick(list(times), lambda c: 1 if c in illegal else 0, time_of, **kw), timed


def test_pick_tie_rules():
    (choice, best, ranked), timed = _pick({'a': 2.0, 'b': 1.0, 'c': 1.0, 'd': 3.0, 'e': 0.5}, illegal=('e',))
    assert (choice, best) == ('b', 1.0)                       # of two equal times the earlier candidate wins
    assert timed == ['a', 'b', 'c', 'd']                      # a candidate whose trial launch fails is never timed nor chosen
    assert ranked == [(1.0, 'b'), (1.0, 'c'), (2.0, 'a')]     # the three fastest
    gemm = dict(better=tuning.faster_by_3_percent, default=1)
    assert _pick({1: 100.0, 2: 98.0}, **gemm)[0][0] == 1      # 2 % faster: the smaller factor stays
    assert _pick({1: 100.0, 2: 96.0}, **gemm)[0][0] == 2      # 4 % faster wins
    for default in (0, (0, 0), 1):
        assert _pick({}, default=default)[0] == (default, None, [])
        assert _pick({'a': 1.0}, illegal=('a',), default=default) == ((default, None, []), [])


def test_tune_records_nothing_without_a_legal_candidate(monkeypatch):
    monkeypatch.setattr(tuning, '_tune_us', {})
    monkeypatch.setattr(tuning, '_tune_top', {})
    assert tuning.tune('wgrad', 'k', [(8, 256)], lambda c: 1, None, default=(0, 0)) == (0, 0)
    assert tuning._tune_us == {} and tuning._tune_top == {}
    assert tuning.tune('conv', 'k', [1, 2, 3, 4], lambda c: 0, {1: 0.004, 2: 0.002, 3: 0.003, 4: 0.002}.get) == 2
    assert tuning._tune_us == {('conv', 'k'): 2.0} and tuning._tune_top == {('conv', 'k'): [(2.0, 2), (2.0, 4), (3.0, 3)]}


@pytest.fixture
def fresh(monkeypatch):
    monkeypatch.setattr(tuning, '_algo_cache', {})
    monkeypatch.setattr(tuning, '_algo_unchecked', set())


class Launch:
    """Stands in for the first launch of a borrowed table entry: records the algo codes it is offered."""

    def __init__(self, rc):
        self.rc, self.seen = rc, []

    def __call__(self, algo):
        self.seen.append(algo)
        return self.rc


def _table_key(pred):
    for key, algo in sorted(plans.conv_entries().items()):
        if key[1] == 8 and pred(tuning.decode(algo)[0], algo):
            return key, algo
    pytest.fail('the shipped table has no such B = 8 conv entry')


def test_table_choice_exact_hit(fresh):
    key, algo = _table_key(lambda fam, algo: algo != 0)
    launch = Launch(0)
    assert tuning.choose_conv('table', key, first_launch=launch) == algo
    assert tuning._algo_cache == {key: algo} and not tuning._algo_unchecked and launch.seen == []


@pytest.mark.parametrize('rc', [0, 1])
def test_table_choice_borrowed_entry_is_checked_by_its_first_launch(fresh, rc):
    key, algo = _table_key(lambda fam, algo: algo != 0)
    other = (key[0], 4) + key[2:]                           # B = 4 borrows the B = 8 tile
    launch = Launch(rc)
    got = tuning.choose_conv('table', other, first_launch=launch)
    assert launch.seen == [algo] and not tuning._algo_unchecked
    if rc == 0:
        assert got is None and tuning._algo_cache == {other: algo}          # the check WAS the launch; the tile stays
    else:
        assert got == 0 and tuning._algo_cache == {other: 0}                # does not fit this batch size: library default
    assert tuning.choose_conv('table', other, first_launch=launch) == (algo if rc == 0 else 0) and launch.seen == [algo]


def test_table_choice_bf16_of_a_winograd_shape(fresh):
    key, algo = _table_key(lambda fam, algo: fam in tuning.WINOGRAD_FAMILIES)
    assert tuning.choose_conv('table', key) == algo
    assert tuning.choose_conv('table', key, bf16=True) == tuning.ALGO_BF16            # library-default tile, bf16 operands
    assert tuning._algo_cache == {key: algo, key + ('bf16',): 0}
    lds, a2 = _table_key(lambda fam, algo: fam in tuning.LDS_WAVES)
    assert tuning.choose_conv('table', lds, bf16=True) == a2 | tuning.ALGO_BF16 and tuning._algo_cache[lds + ('bf16',)] == a2


def test_choice_order_forced_then_cache_then_online(fresh):
    key = (0, 2, 16, 14, 16, 16, 16, 16, False, False)
    asked = []

    def online(k):
        asked.append(k)
        return 0x6011 if len(asked) == 1 else None
    assert tuning.choose_conv(True, key, forced=0x211, online=online) == 0x211 and not asked and not tuning._algo_cache
    assert tuning.choose_conv(True, key, forced=0x611, bf16=True, online=online) == tuning.ALGO_BF16      # forced Winograd tile: no bf16 form
    assert tuning.choose_conv(True, key, forced=0x111, bf16=True) == 0x111 and tuning.choose_conv(True, key, forced=1, bf16=True) == 1
    assert tuning.choose_conv(True, key, online=online) == 0x6011 and tuning._algo_cache == {key: 0x6011}
    assert tuning.choose_conv(True, key, online=online) == 0x6011 and asked == [key]                    # cache hit
    assert tuning.choose_conv(True, key, bf16=True, online=online) == tuning.ALGO_BF16                   # capture: default, not cached
    assert asked == [key, key + ('bf16',)] and key + ('bf16',) not in tuning._algo_cache
    assert tuning.choose_conv(False, key, online=online) == 0
    assert tuning.choose_conv(True, (0, 2, 16, 14, 4, 16, 4, 16, False, False), online=online) == 0 and len(asked) == 2     # small-channel kernels: one form


def test_host_table_pageable_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: False)
    monkeypatch.setattr(torch.Tensor, 'pin_memory', lambda self: self)
    monkeypatch.setattr(torch.Tensor, 'record_stream', lambda self, s: None)

    class Stream:
        device = torch.device('cpu')
    pool, keep = [], []
    tab = ops._HostTable('test table', 24, 3, pool, keep, Stream())
    base = tab.host.data_ptr()
    for i in range(3):
        assert tab.slot() == base + 24 * i
        tab.host[24 * i:24 * (i + 1)] = i + 1
        tab.n += 1
    with pytest.raises(RuntimeError, match='test table: table full'):
        tab.slot()
    tab.n = 2
    dev = tab.upload()
    assert tab.n == 0 and dev.tolist() == [1] * 24 + [2] * 24 and tab.slot() == base
    assert not tab.pinned and keep == [] and pool == []
    words = ops._HostTable('int64 table', 1, 5, pool, keep, Stream(), torch.int64)
    words.n = 1
    assert words.capacity == 5 and words.slot() == words.host.data_ptr() + 8
