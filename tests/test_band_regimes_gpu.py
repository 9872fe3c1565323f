"""conv3x3_lds_k, the persistent 3x3 band kernel, through the C ABI at every launch regime of tests/band_cases.py: the integer problem
against the int64 convolution with `==` (bf16 operands included), the float problem against float64 under the derived per-element bound
(bit 20: of the bf16-rounded operands, with 2K for K), inputs in NaN-padded buffers, destinations whose padding must come back
bit-unchanged, the fused forward and backward BatchNorm statistics against float64 sums of the device's own output; the bit identities
the kernel documents (every forced (NW, NT, MTW, TH) equals 0x211, the default equals the forced tile the mirror says it chose, the fused
statistics do not change `out`, bit 20 is ignored at R = 2, a launch repeats) and the refusals.  The buffers, the argument list and the
comparisons are those of test_conv_regimes_gpu.py; every measured ratio error / bound is appended to conv_errors.jsonl."""
import pytest

import band_cases as bc
import conv_cases as cc
import test_conv_regimes_gpu as tg
from test_conv_regimes_gpu import run, same_bits, variant

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('kind', ['int', 'float'])
@pytest.mark.parametrize('name', bc.RUN_CASES)
def test_band_case(dev, name, kind):
    case = bc.CASES[name]
    pr = cc.problem(case, kind)
    out, sums = run(dev, pr)
    ratio = cc.compare(pr, out)
    print(name, kind, ratio)
    cc.check('rv_conv_fwd ' + kind, case['name'], 'out', ratio, log=True)
    assert (sums is not None) == bool(case['stats'])
    if sums is not None:
        cc.check('rv_conv_fwd ' + kind, case['name'], 'stats', cc.stats_ratio(pr, out, sums), log=True)


# ---------------------------------------------------------------------------------------------------------------------
# bit identities (the float problem)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [n for n in bc.FORCED_CASES if bc.CASES[n]['W'] <= 64 and bc.CASES[n]['algo'] & ~bc.BF16_BIT != 0x211])
def test_every_forced_tile_equals_0x211(dev, name):
    """each output element is one chain ordered by chunk, then tap, then k, wherever its lane sits and however the bands are cut and dealt to workgroups"""
    case = bc.CASES[name]
    pr = cc.problem(case, 'float')
    assert cc.case_regime(dict(case, algo=bc.base_algo(case)))['tile'] == (1, 1)
    assert same_bits(run(dev, pr)[0], run(dev, pr, algo=bc.base_algo(case))[0])


@pytest.mark.parametrize('name', bc.DEFAULT_CASES)
def test_default_equals_the_tile_the_mirror_chose(dev, name):
    case = bc.CASES[name]
    reg = cc.case_regime(case)
    algo = bc.forced(4, reg['tile'][0], reg['tile'][1], reg['TH'], reg['bf'])
    same = cc.case_regime(dict(case, algo=algo))
    assert all(same[k] == reg[k] for k in ('tile', 'TH', 'wgs_per_cu', 'grid', 'bands_per_wg', 'lds_bytes'))
    pr = cc.problem(case, 'float')
    assert same_bits(run(dev, pr)[0], run(dev, pr, algo=algo)[0])


@pytest.mark.parametrize('name', [n for n in bc.BAND_CASES if bc.CASES[n]['stats']])
def test_fused_statistics_do_not_change_out(dev, name):
    case = bc.CASES[name]
    assert same_bits(run(dev, cc.problem(case, 'float'))[0], run(dev, cc.problem(variant(case, 'no statistics', stats=None), 'float'))[0])


def test_bf16_bit_is_ignored_at_R2(dev):
    case = bc.CASES['bf16 ignored R2 8->16']
    pr = cc.problem(case, 'float')
    assert case['algo'] & bc.BF16_BIT and same_bits(run(dev, pr)[0], run(dev, pr, algo=case['algo'] & ~bc.BF16_BIT)[0])


@pytest.mark.parametrize('name', [n for i, n in enumerate(bc.BAND_CASES) if i % 3 == 0 or n.split()[0] in ('run', 'default', 'bf16')])
def test_launch_repeats_bit_for_bit(dev, name):
    pr = cc.problem(bc.CASES[name], 'float')
    (out1, sums1), (out2, sums2) = run(dev, pr), run(dev, pr)
    assert same_bits(out1, out2)
    if sums1 is not None and cc.case_regime(bc.CASES[name])['grid'] <= cc.RV_BN_NREP:      # one workgroup per replica: no order of atomics to differ in
        assert same_bits(sums1, sums2)


# ---------------------------------------------------------------------------------------------------------------------
# refusals: non-zero, a message, the destinations untouched; the same buffers then serve an accepted call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', bc.REFUSED_CASES)
def test_refused_case(dev, name):
    case = bc.CASES[name]
    pr = cc.problem(case, 'float')
    d = tg.upload(dev, pr)
    tg._refused(d, tg.conv_args(pr, d), name)
    ok = dict(case, name=case['name'] + ' / default', algo=0, refusal=None)
    assert cc.case_regime(ok)['kernel'] == 'band'
    tg._lib().call('rv_conv_fwd', *tg.conv_args(pr, d, algo=0))
    out, _ = tg.collect(pr, d)
    cc.check('rv_conv_fwd after a refusal', ok['name'], 'out', cc.compare(cc.problem(ok, 'float'), out))


def test_band_refusals(dev):
    name = 'default 32->48'                                          # 2 x 3 x 33, 32 -> 48 with forward statistics
    case = bc.CASES[name]
    pr = cc.problem(case, 'float')
    d = tg.upload(dev, pr)
    ok = tg.conv_args(pr, d)
    for what, kw in (('NT = 2 against three n-tiles', {'algo': 0x221}), ('NT = 4 against three n-tiles', {'algo': 0x441}), ('12 waves (3, 2)', {'algo': 0x732}),
                     ('MTW = 3 at four waves', {'algo': 0x213}), ('MTW = 8 at twelve waves', {'algo': 0x718}), ('3 rows where the slots hold 1', {'algo': 0x3211}),
                     ('16 waves (3, 4)', {'algo': 0x434}), ('bf16 on a refused tile', {'algo': 0x221 | bc.BF16_BIT}), ('in 4 bytes off', {'in': ok[1] + 4}),
                     ('in_ld odd', {'in_ld': 33, 'algo': 0x211}), ('bn_z without bn_coef', {'bn_z': ok[1], 'bn_z_ld': 48})):
        assert what.startswith('in') or what.startswith('bn_z') or cc.case_regime(dict(case, **kw)).get('refused'), what
        tg._refused(d, tg.conv_args(pr, d, **kw), what)
    tg._lib().call('rv_conv_fwd', *ok)
    out, sums = tg.collect(pr, d)
    cc.check('rv_conv_fwd after refusals', case['name'], 'out', cc.compare(pr, out))
    cc.check('rv_conv_fwd after refusals', case['name'], 'stats', cc.stats_ratio(pr, out, sums))
