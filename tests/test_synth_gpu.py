"""The synthesiser on the device (rv_synth_render) against the float64 definition `synth.render_host`.

Bound, derived and not measured, for rows with e + R - s <= 2^24 (so that t and t + 1 are exact in float32):

    |y - y64| <= 32 u S[n] + u E[n],   u = 2^-24,   S[n] = sum amp att decay rel,   E[n] = sum amp att rel.

A rounding to float32 costs a relative u at most.  Per term, in the kernel's arithmetic:
    theta      exact (uint32).  Read as a signed int32 v (|v| <= 2^31) and converted to float: off by at most 2^6 units = 2^-26 turn;
               the scaling by 2^-31 is exact; sin(pi x) has slope pi per half turn, so osc is off by pi 2^-25 = 1.57 u at most
    sinpif     4 ulp of a value below 1 (the OpenCL limit; the device library documents less):                        4 u
    expf       3 ulp (the OpenCL limit), an ulp being 2 u of the value at most:                                       6 u
    dec * t    one rounding of the argument x = dec t: x u e^-x <= 0.37 u of amp att rel -- the E term, with room to spare
    att        min(t + 1, A) and A exact up to 2^24, one correctly rounded division:                                  1 u
               (an A above 2^24 costs one more for its conversion)
    rel        e + R - n and R exact up to 2^24, one division, one square: 2 * 1 + 1 =                                3 u
               (an R above 2^24: two more roundings before the square, 4 u more)
    products   amp att, decay, rel, osc:                                                                              4 u
    sum        float64: 2^-53 per add, nothing at this scale; the float32 output is one rounding of y:                1 u
That is 20.6 u of S for the rows `partials` makes (25.6 u with A and R beyond 2^24) and 0.37 u of E, first order; the rest of the
32 u of S is second-order slack.  Nothing depends on the number of rows that sound at once -- the 300-row case shows it.  An
exponent beyond the float32 range (dec t = 200) gives 0 where the exact value is below 2^-126: inside u E.  int16 is the rounding
of the float64 sum itself, so it lies within 1 LSB of the yardstick's wherever 32768 bound < 1.  No sample is excluded.

Every raw call writes into a buffer with 37 elements of a sentinel on either side, which must survive."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from reconvat_amd import synth
from reconvat_amd.constants import HOP_LENGTH
from test_synth import row

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 37
SENTINEL = {torch.float32: -12345.5, torch.int16: -12345}
DTYPES = [torch.float32, torch.int16]
U32 = 1 << 32
N_TILES = 6
SPANS = [(0, 1), (0, 1023), (0, 1024), (0, 1025), (0, 4099), (1000, 2100), (1024, 1024), (3071, 2), (4000, 2144)]


def raw(rows, tile_ptr, tile_rows, n_tiles, n0, n_out, dtype, expect=0):
    """rv_synth_render into a guarded buffer; returns y [n_out] (numpy) after checking the guards -- or, for an expected failure, that
    nothing at all was written."""
    from reconvat_amd import _lib
    from reconvat_amd._lib import ptr
    dev = torch.device('cuda:0')
    up = lambda a, t: None if a is None or len(a) == 0 else torch.from_numpy(np.asarray(a, dtype=t).view(np.int32).reshape(-1)).to(dev)
    d_rows, d_ptr, d_list = up(rows, np.uint32), up(tile_ptr, np.int32), up(tile_rows, np.int32)
    buf = torch.full((n_out + 2 * GAP,), SENTINEL[dtype], device=dev, dtype=dtype)
    rc = _lib.load().rv_synth_render(ptr(d_rows), 0 if rows is None else len(rows), ptr(d_ptr), ptr(d_list), n_tiles, n0, n_out,
                                     buf.data_ptr() + GAP * buf.element_size(), synth.OUT_DTYPES[dtype], None)
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    if expect != 0:
        assert rc == expect and 'rv_synth_render' in _lib.last_error()
        assert np.all(out == SENTINEL[dtype]), 'a refused call wrote'
        return None
    assert rc == 0, _lib.last_error()
    assert np.all(out[:GAP] == SENTINEL[dtype]) and np.all(out[GAP + n_out:] == SENTINEL[dtype]), 'a store left the output'
    return out[GAP:GAP + n_out].copy()


def check(y, rows, n0, n_out, dtype, tag):
    y64 = synth.render_host(rows, n0, n_out)
    bound = synth.error_bound(rows, n0, n_out)
    if dtype == torch.int16:
        assert 32768 * bound.max() < 1, tag
        diff = np.abs(y.astype(np.int64) - synth.to_int16(y64).astype(np.int64))
        print(f'{tag}: {int((diff != 0).sum())} of {n_out} samples one LSB off')
        assert diff.max() <= 1, (tag, int(np.argmax(diff)))
        return
    err = np.abs(y.astype(np.float64) - y64)
    print(f'{tag}: worst |y - y64| / bound {np.max(err / np.maximum(bound, 1e-300)):.4f}')
    assert np.all(err <= bound), (tag, int(np.argmax(err - bound)))


def table():
    """The hand-made table: six tiles; tile 4 = [4096, 5120) is empty between two occupied ones."""
    rs = np.random.RandomState(12)
    rows = [
        row(0, 2100, 0x1234567, 99, 0.05, 0.1, 48, 40),                  # dec t reaches 210: the tail is an exact zero
        row(50, 60, 1 << 31, 777, 0.05, 0.0, 1, 1),                      # A = 1 and R = 1; half a turn per sample
        row(100, 900, 1, 1 << 29, 0.05, 0.0, 48, 1600),                  # inc = 1; wholly in its release from 900 to 2500
        row(200, 1000, U32 - 1, 5, 0.05, 1e-3, 640, 24),                 # ends exactly at 1024 (e + R); inc = 2^32 - 1
        row(900, 3200, 0x0B43958F, 0xFFFFFF00, 0.05, 2e-4, 48, 100),     # spans three tiles (and a fourth); the phase wraps at once
        row(1024, 1500, 0, 1 << 30, 0.05, 0.0, 640, 1280),               # starts exactly at 1024; inc = 0: its envelope alone
        row(1023, 1025, 0x30000000, 0, 0.05, 0.0, 3, 2),                 # two samples across a tile boundary
        row(3000, 3080, 0x7FFFFFFF, 0x80000000, 0.05, 5e-3, 7, 5),
        row(5200, 5600, 0x10000001, 42, 0.05, 1e-3, 48, 300),            # behind the empty tile
    ]
    for _ in range(300):                                                 # 300 rows on the same samples
        rows.append(row(1100 + int(rs.randint(0, 3)), 1900, int(rs.randint(0, U32, dtype=np.int64)), int(rs.randint(0, U32, dtype=np.int64)),
                        0.001 * rs.uniform(0.5, 1.0), rs.choice([0.0, 1e-3, 1e-2]), int(rs.choice([1, 48, 640])), int(rs.choice([1, 160, 300]))))
    rows = np.stack(rows)
    rows = rows[np.argsort(rows[:, 0].view(np.int32), kind='stable')]
    tile_ptr, tile_rows = synth.tile_lists(rows, N_TILES)
    assert tile_ptr[4] == tile_ptr[5] and tile_ptr[3] < tile_ptr[4] and tile_ptr[5] < tile_ptr[6]
    return rows, tile_ptr, tile_rows


@pytest.fixture(scope='module')
def hand():
    return table()


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'i16'])
@pytest.mark.parametrize('n0,n_out', SPANS)
def test_raw_entry_point_stays_within_the_bound(dev, hand, n0, n_out, dtype):
    rows, tile_ptr, tile_rows = hand
    y = raw(rows, tile_ptr, tile_rows, N_TILES, n0, n_out, dtype)
    check(y, rows, n0, n_out, dtype, f'[{n0}, {n0} + {n_out}) {dtype}')
    if n0 + n_out > 4096:
        lo, hi = max(n0, 4096), min(n0 + n_out, 5120)
        assert np.all(y[lo - n0:hi - n0] == 0)                           # the empty tile


def test_the_bound_does_not_grow_with_the_row_count(dev, hand):
    """Samples 1200 .. 1800 carry 300 rows more than their neighbours: the worst error relative to the bound is of the same size
    there as on the nine-row remainder (a float32 running sum would grow with the count), and at most 1."""
    rows, tile_ptr, tile_rows = hand
    y = raw(rows, tile_ptr, tile_rows, N_TILES, 0, 4096, torch.float32)
    ratio = np.abs(y - synth.render_host(rows, 0, 4096)) / np.maximum(synth.error_bound(rows, 0, 4096), 1e-300)
    print(f'crowded {ratio[1200:1800].max():.4f}, elsewhere {max(ratio[:1100].max(), ratio[2000:].max()):.4f}')
    assert ratio.max() <= 1


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'i16'])
def test_degenerate_calls(dev, hand, dtype):
    rows, tile_ptr, tile_rows = hand
    zeros = raw(None, np.zeros(N_TILES + 1, dtype=np.int32), None, N_TILES, 1000, 2100, dtype)
    assert np.all(zeros == 0)
    # entries outside [0, n_rows) in front of, inside and behind every list: the result is that of the table without them
    want = raw(rows, tile_ptr, tile_rows, N_TILES, 0, N_TILES * 1024, dtype)
    ptr2, list2 = [0], []
    for j in range(N_TILES):
        mine = list(tile_rows[tile_ptr[j]:tile_ptr[j + 1]])
        mine = [-1] + mine[:len(mine) // 2] + [len(rows), -7, 2 ** 31 - 1] + mine[len(mine) // 2:] + [len(rows)]
        list2 += mine
        ptr2.append(len(list2))
    got = raw(rows, ptr2, list2, N_TILES, 0, N_TILES * 1024, dtype)
    assert np.array_equal(got.view(np.uint32 if dtype == torch.float32 else np.int16), want.view(np.uint32 if dtype == torch.float32 else np.int16))
    # a call that reaches past the table's tiles is refused, and writes nothing
    raw(rows, tile_ptr, tile_rows, N_TILES, N_TILES * 1024 - 10, 11, dtype, expect=-1)
    raw(rows, tile_ptr, tile_rows, N_TILES, N_TILES * 1024 + 1, 1, dtype, expect=-1)
    raw(rows, tile_ptr, tile_rows, N_TILES, -1, 10, dtype, expect=-1)
    last = raw(rows, tile_ptr, tile_rows, N_TILES, N_TILES * 1024 - 10, 10, dtype)
    assert np.array_equal(last, want[-10:])


def test_int16_rounding_and_saturation(dev):
    """DC rows (inc = 0, a quarter turn: osc = +-1, A = R = 1, dec = 0) of amp = (k + 0.5) / 32768: every factor but amp is exactly
    1, 32768 y = k + 0.5 exactly, and the result is the even neighbour; amp = 2 saturates."""
    ks = [0, 1, 2, 3, 100, 101, 12344, 12345, 32766]
    rows, want = [], []
    for i, k in enumerate(ks):
        for sign, ph in ((1, 1 << 30), (-1, 3 << 30)):
            at = 20 * (2 * i + (sign < 0))
            rows.append(row(at, at + 5, 0, ph, (k + 0.5) / 32768, 0.0, 1, 1))
            want.append((at, int(np.rint(sign * (k + 0.5)))))
    rows.append(row(600, 605, 0, 1 << 30, 2.0, 0.0, 1, 1))
    rows.append(row(620, 625, 0, 3 << 30, 2.0, 0.0, 1, 1))
    want += [(600, 32767), (620, -32768)]
    rows = np.stack(rows)
    tile_ptr, tile_rows = synth.tile_lists(rows, 1)
    y = raw(rows, tile_ptr, tile_rows, 1, 0, 1024, torch.int16)
    expect = np.zeros(1024, dtype=np.int16)
    for at, v in want:
        expect[at:at + 6] = v                                             # five samples and the one-sample release at rel = 1
    assert np.array_equal(y, expect)
    assert np.array_equal(y, synth.to_int16(synth.render_host(rows, 0, 1024)))
    f = raw(rows, tile_ptr, tile_rows, 1, 0, 1024, torch.float32)
    assert f[600] == 2.0 and f[620] == -2.0 and f[0] == np.float32(0.5 / 32768)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'i16'])
def test_cuts_do_not_change_a_bit(dev, hand, dtype):
    rows, tile_ptr, tile_rows = hand
    whole = raw(rows, tile_ptr, tile_rows, N_TILES, 0, 5000, dtype)
    cuts = [0, 1, 1024, 3000, 5000]
    parts = np.concatenate([raw(rows, tile_ptr, tile_rows, N_TILES, a, b - a, dtype) for a, b in zip(cuts[:-1], cuts[1:])])
    view = np.uint32 if dtype == torch.float32 else np.int16
    assert np.array_equal(parts.view(view), whole.view(view)) and np.abs(whole.astype(np.float64)).max() > 0


@pytest.mark.parametrize('voice', ['struck', 'sustained'])
@pytest.mark.parametrize('seed', [0, 1])
def test_a_real_score(dev, seed, voice):
    notes = synth.random_score(np.random.RandomState(seed), 4.0)
    timbre = synth.Timbre(voice, seed)
    rows = synth.partials(notes, timbre)
    n = 4 * 16000
    assert len(notes) >= 1
    for dtype in DTYPES:
        y = synth.render(notes, n, timbre, device=dev, out_dtype=dtype)
        assert y.device.type == 'cuda' and y.dtype == dtype and y.shape == (n,)
        check(y.cpu().numpy(), rows, 0, n, dtype, f'score {seed} {voice} {dtype}')
        assert torch.equal(synth.render(rows, n, device=dev, out_dtype=dtype), y)       # the table itself is accepted too
    host = synth.render(notes, n, timbre, device='cpu', out_dtype=torch.int16)
    assert int((host.int() - y.cpu().int()).abs().max()) <= 1 and int(host.abs().max()) > 300


def test_render_cuts_long_signals(dev, monkeypatch):
    notes = synth.random_score(np.random.RandomState(3), 5.0)
    timbre = synth.Timbre('struck', 3)
    whole = synth.render(notes, 80000, timbre, device=dev, out_dtype=torch.float32)
    monkeypatch.setattr(synth, 'CHUNK', 3 * 1024)
    assert torch.equal(synth.render(notes, 80000, timbre, device=dev, out_dtype=torch.float32), whole)
    assert synth.render(notes, 0, timbre, device=dev).shape == (0,)


def test_rendered_tracks_feed_the_device_corpus(dev):
    from reconvat_amd.dataset import RenderedScores, crop_item
    from reconvat_amd.feed import DeviceCorpus
    seq, n = 32768, 2 * 32768 + 16 * HOP_LENGTH                         # 4.6 s: a score's events fall in 0.5 .. 1.6 s
    on_dev = RenderedScores(3, n, ('struck', 'sustained'), seed=8, device=dev, sequence_length=seq)
    on_host = RenderedScores(3, n, ('struck', 'sustained'), seed=8, device='cpu', sequence_length=seq)
    for a, b in zip(on_dev.data, on_host.data):
        assert a['path'] == b['path'] and torch.equal(a['label'], b['label']) and torch.equal(a['velocity'], b['velocity'])
        assert a['audio'].dtype == torch.int16 and not a['audio'].is_cuda
        assert int((a['audio'].int() - b['audio'].int()).abs().max()) <= 1 and int(a['audio'].abs().max()) > 300
    order = [2, 0, 1]
    out = DeviceCorpus(on_dev.data, seq, 3, dev, seed=42).batch(order)
    for b, i in enumerate(order):
        item = crop_item(on_host.data[i], int(out['start_idx'][b]) // HOP_LENGTH, seq)
        assert torch.equal(out['frame'][b].cpu(), item['frame']) and torch.equal(out['onset'][b].cpu(), item['onset'])
        assert torch.equal(out['audio'][b].cpu(), crop_item(on_dev.data[i], int(out['start_idx'][b]) // HOP_LENGTH, seq)['audio'])
    item = on_dev[0]
    assert item['audio'].shape == (seq,) and item['frame'].shape == (seq // HOP_LENGTH, 88)


def test_command_line_run_on_the_rendered_corpus(dev, tmp_path):
    """`train_UNet_VAT.py with train_on=Rendered ...`: two steps on the tiny rendered corpus."""
    logdir = str(tmp_path / 'rendered')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train_UNet_VAT.py'), 'with', 'train_on=Rendered', 'small=True', 'supersmall=True',
                        'sequence_length=32768', 'batch_size=2', 'train_batch_size=2', 'iteration=2', 'epoches=1', f'logdir={logdir}'],
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + '\n---\n' + p.stderr[-3000:]
    assert 'Training finished.' in p.stdout
    with open(os.path.join(logdir, 'corpus_rank0.json')) as fh:
        corpus = json.load(fh)
    assert corpus['train_on'] == 'Rendered' and len(corpus['labelled']) == 4 and len(corpus['unlabelled']) == 16
    for key in ('labelled', 'unlabelled', 'labelled_shard', 'unlabelled_shard', 'validation', 'full_validation'):
        assert corpus[key] and all(path.startswith('rendered/') for path in corpus[key]), key
    with open(os.path.join(logdir, 'scalars.jsonl')) as fh:
        losses = [r['value'] for r in map(json.loads, fh) if r['tag'].startswith('loss/train_')]
    assert len(losses) >= 3 and np.all(np.isfinite(losses)), losses


def test_transcribe_files_writes_a_rendering(dev, tmp_path):
    import transcribe_files
    n = 2 * 16000
    src, out = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    transcribe_files.write_rendering(str(src / 'tune.wav'), [[0.2, 1.0, 60, 100], [0.6, 1.4, 67, 90]], n, dev)
    with wave.open(str(src / 'tune.wav'), 'rb') as w:
        assert (w.getnframes(), w.getframerate(), w.getsampwidth(), w.getnchannels()) == (n, 16000, 2, 1)
        assert np.abs(np.frombuffer(w.readframes(n), dtype='<i2')).max() > 300
    transcribe_files.main(['with', f'input={src}', f'output={out}', 'render=True', 'device=cuda:0'])
    assert sorted(os.listdir(out)) == ['ReconVAT-tune.mid', 'ReconVAT-tune.wav']
    with wave.open(str(out / 'ReconVAT-tune.wav'), 'rb') as w:
        assert (w.getnframes(), w.getframerate(), w.getsampwidth(), w.getnchannels()) == (n, 16000, 2, 1)
    transcribe_files.main(['with', f'input={src}', f'output={tmp_path / "plain"}', 'device=cuda:0'])
    assert os.listdir(tmp_path / 'plain') == ['ReconVAT-tune.mid']                     # off by default
