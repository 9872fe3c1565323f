"""Sub-frame note onsets on the device (csrc/onset_time.hip): rv_onset_refine against the host definition
(reconvat_amd/onset_time.py).  The amplitudes stay within the float32 bound derived in tests/onset_time_cases.py; the sample equals the
host's on every note the bound makes safe, and on EVERY note it equals the definition's vote applied to the kernel's own amplitudes
(float32 differences, first maximum, lower median, clamp: integers, ==).  Then order independence, the argument checks and the layers
above: transcribe2midi(refine_onsets=True) and evaluate_timing."""
import os
import sys

import numpy as np
import pytest
import torch

import onset_time_cases as oc
from reconvat_amd import onset_time as ot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_run(dev, audio, keys, frames, lead=0):
    x = audio if torch.is_tensor(audio) else torch.from_numpy(np.array(audio)).to(dev)
    out, amp = ot.refine_device(x, keys, frames, lead, return_amplitudes=True)
    assert out.dtype == torch.int32 and out.shape == (len(keys),) and amp.dtype == torch.float32 and amp.shape == (len(keys), 49, 8)
    assert out.device == x.device and amp.device == x.device
    return out.cpu().numpy().astype(np.int64), amp.cpu().numpy()


def check(dev, audio, keys, frames, lead=0, reference=None, tag=''):
    """The kernel on (audio, notes) against the definition; returns (samples, amplitudes) of the device."""
    keys, frames = np.asarray(keys, dtype=np.int64), np.asarray(frames, dtype=np.int64)
    host = audio.cpu().numpy() if torch.is_tensor(audio) else audio
    got, amp = device_run(dev, audio, keys, frames, lead)
    if reference is None:
        A, bound = oc.amp_bound(host, keys, frames)
        reference = A, bound, oc.safe_notes(A, bound, keys), None
    A, bound, safe, _ = reference
    err = np.abs(amp.astype(np.float64) - A)
    print(f'{tag}: {len(keys)} notes, worst |A - A64| / bound {np.max(err / bound):.4f}, {int(safe.sum())} safe')
    assert np.all(err <= bound), (tag, np.unravel_index(np.argmax(err - bound), err.shape))
    invalid = np.arange(8)[None, :] >= ot.valid_harmonics()[keys][:, None]
    assert np.all(amp[np.broadcast_to(invalid[:, None, :], amp.shape)] == 0)
    want = ot.refine_host(host, keys, frames, lead)
    print(f'{tag}: the sample differs from the host\'s on {int((got != want).sum())} notes, none of them safe')
    assert np.array_equal(got[safe], want[safe]), (tag, np.flatnonzero(safe & (got != want))[:5])
    # every note, exactly: the vote of the definition on the kernel's own float32 amplitudes
    own = ot._samples(ot.pick(amp, keys), frames, lead, len(host))
    assert np.array_equal(got, own), (tag, np.flatnonzero(got != own)[:5])
    assert np.all((got >= 0) & (got < len(host)))
    return got, amp


# ---- 5. amplitudes and samples ---------------------------------------------------------------------------------------------------------
def test_parity_input(dev):
    audio, keys, frames = oc.parity_input()
    check(dev, audio, keys, frames, reference=oc.parity_reference(), tag='8 s struck seed 0 + hand-placed notes')


@pytest.mark.parametrize('n', [1, 2, 257])
def test_note_counts(dev, n):
    audio, keys, frames = oc.parity_input()
    A, bound, safe, _ = oc.parity_reference()
    idx = (np.arange(n) * 7 + 3) % len(keys)                            # 257 > the list: notes repeat
    check(dev, audio, keys[idx], frames[idx], reference=(A[idx], bound[idx], safe[idx], None), tag=f'n = {n}')


@pytest.mark.parametrize('lead', [320, 100000])
def test_lead(dev, lead):
    audio, keys, frames = oc.parity_input()
    got, _ = check(dev, audio, keys, frames, lead=lead, reference=oc.parity_reference(), tag=f'lead {lead}')
    assert (got == 0).any()                                             # clamped at the first sample


def test_audio_shorter_than_one_window(dev):
    audio, keys, frames = oc.parity_input()
    first = int(frames[3]) * 512 - 700                                  # T = 2000 < 2048 around a true onset
    clip = np.ascontiguousarray(audio[first:first + 2000])
    k = np.array([keys[3], keys[3], keys[3], keys[3], 0, 87, keys[4]])
    t = np.array([0, 1, 2, 3, 1, 1, 40])
    got, amp = check(dev, clip, k, t, tag='T = 2000')
    assert amp[:4].max() > 0.1 and np.all(amp[6] == 0) and got[6] == 1999


def test_audio_pointer_offset_by_one_float(dev):
    audio, keys, frames = oc.parity_input()
    base = torch.from_numpy(np.array(audio)).to(dev)
    view = base[1:]
    assert view.data_ptr() == base.data_ptr() + 4 and view.is_contiguous()
    check(dev, view, keys, frames, tag='audio + 1')


def test_every_key(dev):
    audio, keys, frames = oc.parity_input()
    t = int(frames[len(frames) // 2])
    check(dev, audio, np.arange(88), np.full(88, t), tag='keys 0..87')


def test_known_answers(dev):
    """The impulse case of tests/test_onset_time.py: every amplitude is one window value, the sample is s0 - 128."""
    audio = np.zeros(40 * 512, np.float32)
    frames, k0 = np.array([4, 12, 20, 28, 36]), np.array([24, 10, 40, 5, 31])
    s0 = 512 * frames - 768 + 32 * k0
    audio[s0] = 1.0
    for key in (0, 39, 87):
        got, _ = check(dev, audio, np.full(5, key), frames, tag=f'impulses, key {key}')
        assert np.array_equal(got, s0 - 128)


# ---- 6. order independence -------------------------------------------------------------------------------------------------------------
def test_same_bytes_for_any_order(dev):
    audio, keys, frames = oc.parity_input()
    x = torch.from_numpy(np.array(audio)).to(dev)
    s0, a0 = device_run(dev, x, keys, frames)
    s1, a1 = device_run(dev, x, keys, frames)
    assert s0.tobytes() == s1.tobytes() and a0.tobytes() == a1.tobytes()
    perm = np.random.RandomState(3).permutation(len(keys))
    sp, ap = device_run(dev, x, keys[perm], frames[perm])
    assert sp.tobytes() == s0[perm].tobytes() and ap.tobytes() == a0[perm].tobytes()
    for i in (0, 17, len(keys) - 1):
        si, ai = device_run(dev, x, keys[i:i + 1], frames[i:i + 1])
        assert si.tobytes() == s0[i:i + 1].tobytes() and ai.tobytes() == a0[i:i + 1].tobytes(), i
    only = ot.refine_device(x, keys, frames)                            # without the amplitudes
    assert only.dtype == torch.int32 and np.array_equal(only.cpu().numpy(), s0)
    assert np.array_equal(ot.refine(x, keys, frames), s0) and ot.refine(x, keys, frames).dtype == np.int64


# ---- 7. argument handling --------------------------------------------------------------------------------------------------------------
def test_arguments(dev):
    from reconvat_amd import _lib
    audio, keys, frames = oc.parity_input()
    x = torch.from_numpy(np.array(audio)).to(dev)
    out = ot.refine_device(x, [], [])
    assert out.shape == (0,) and out.dtype == torch.int32
    assert ot.refine_intervals(x, [], np.zeros((0, 2)), device=True).shape == (0, 2)
    table = ot.device_table(dev)
    assert table is ot.device_table(dev) and table.shape == (88, 8, 2, 512) and table.data_ptr() % 16 == 0
    notes = torch.tensor([[40, 10], [41, 11]], dtype=torch.int32, device=dev)
    res = torch.full((2,), -7, dtype=torch.int32, device=dev)
    raw = lambda *a: _lib.invoke('rv_onset_refine', *a, _lib.stream())
    # n = 0 launches nothing, whatever the pointers are
    assert raw(None, len(audio), None, None, 0, 0, None, None) == 0
    for bad in ((x.data_ptr(), len(audio), table.data_ptr(), notes.data_ptr(), 2, -1, res.data_ptr(), None),          # negative lead
                (x.data_ptr(), 0, table.data_ptr(), notes.data_ptr(), 2, 0, res.data_ptr(), None),                    # no audio
                (x.data_ptr(), len(audio), table.data_ptr(), notes.data_ptr(), -1, 0, res.data_ptr(), None),          # negative n
                (None, len(audio), table.data_ptr(), notes.data_ptr(), 2, 0, res.data_ptr(), None),                   # null pointer
                (x.data_ptr(), len(audio), table.data_ptr() + 4, notes.data_ptr(), 2, 0, res.data_ptr(), None),       # misaligned table
                (x.data_ptr(), len(audio), table.data_ptr(), notes.data_ptr(), 2, 0, res.data_ptr() + 2, None)):      # misaligned output
        assert raw(*bad) != 0 and 'rv_onset_refine' in _lib.last_error()
    torch.cuda.synchronize()
    assert res.tolist() == [-7, -7]                                     # nothing was launched
    # a row that is not a note is marked by the kernel and reads no table
    rows = torch.tensor([[40, 10], [88, 10], [-1, 10], [40, -1], [40, 1 << 22], [41, 11]], dtype=torch.int32, device=dev)
    res = torch.full((6,), -7, dtype=torch.int32, device=dev)
    amp = torch.full((6, 49, 8), -7.0, device=dev)
    assert raw(x.data_ptr(), len(audio), table.data_ptr(), rows.data_ptr(), 6, 0, res.data_ptr(), amp.data_ptr()) == 0
    want = ot.refine_host(audio, [40, 41], [10, 11])
    safe = oc.safe_notes(*oc.amp_bound(audio, [40, 41], [10, 11]), np.array([40, 41]))
    got = res.cpu().numpy()
    assert got[1:5].tolist() == [-1] * 4 and bool((amp[1:5] == 0).all()) and np.all((got[[0, 5]] == want) | ~safe)
    assert np.array_equal(got[[0, 5]], ot._samples(ot.pick(amp[[0, 5]].cpu().numpy(), [40, 41]), np.array([10, 11]), 0, len(audio)))
    # the Python layer raises before it launches
    for k, t in (([88], [1]), ([-1], [1]), ([3], [-1]), ([3, 4], [1])):
        with pytest.raises(ValueError):
            ot.refine_device(x, k, t)
    with pytest.raises(ValueError):
        ot.refine_device(x, [3], [1], lead=-1)
    with pytest.raises(ValueError):
        ot.refine_device(x.double(), [3], [1])
    with pytest.raises(RuntimeError, match='HIP device only'):
        ot.refine_device(x.cpu(), [3], [1])
    with pytest.raises(RuntimeError, match='HIP device only'):
        ot.refine_intervals(x.cpu(), [3], [[1, 2]], device=True)


# ---- 8. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def onset_model(dev):
    import reconvat_amd as ra
    from oracle import fixture as fx
    m = ra.UNet_Onset((2, 2), (2, 2), log=True, reconstruction=True, mode='imagewise', spec='Mel')
    m.load_state_dict(fx.fixture_params('onset', True))
    return m.to(dev).eval()


def fixture_thresholds(model, audio):
    """The weights are a fixture, not a trained model: thresholds from the posteriorgrams themselves, so that there are notes to decode."""
    with torch.no_grad():
        pred = model.transcribe({'audio': audio.unsqueeze(0)})
    onset, frame = pred['onset'].squeeze(0).relu().cpu(), pred['frame'].squeeze(0).relu().cpu()
    return onset, frame, float(onset.flatten().quantile(0.97)), float(frame.flatten().quantile(0.9))


def test_transcribe2midi_with_refined_onsets(dev, onset_model, tmp_path):
    sys.path.insert(0, ROOT)
    import transcribe_files as tf
    from reconvat_amd import decoding as md
    from reconvat_amd.evaluate import midi_to_hz
    from reconvat_amd.midi import parse_midi, save_midi
    audio, _ = oc.rendered('struck', 0, 8)
    pcm = torch.from_numpy(np.rint(audio[8000:8000 + 128 * 512] * 32768.0).astype(np.int16))
    clip = tmp_path / 'clip.pt'
    torch.save({'audio': pcm}, str(clip))
    x = tf.load_audio(str(clip))
    onset, frame, thr_on, thr_fr = fixture_thresholds(onset_model, x.to(dev))
    p_est, i_est = md.extract_notes_wo_velocity(onset, frame, thr_on, thr_fr, rule='rule2', min_frames=2)
    assert len(p_est) > 5
    for lead, name in ((0, 'plain'), (48, 'lead')):
        tf.transcribe2midi([str(clip)], onset_model, dev, str(tmp_path / name), onset_threshold=thr_on, frame_threshold=thr_fr,
                           min_frames=2, refine_onsets=True, onset_lead=lead)
        want_iv = ot.refine_intervals(x.numpy(), p_est, i_est, lead)                         # the host path
        save_midi(str(tmp_path / f'{name}.mid'), np.array([midi_to_hz(21 + q) for q in p_est]), want_iv, [127] * len(p_est))
        got, want = parse_midi(str(tmp_path / name / 'ReconVAT-clip.mid')), parse_midi(str(tmp_path / f'{name}.mid'))
        assert got.shape == want.shape == (len(p_est), 4) and np.array_equal(got, want), lead
    # ... and they are not the frame grid's
    grid = np.asarray(i_est).reshape(-1, 2)[:, 0] * 512 / 16000
    assert np.abs(np.sort(want_iv[:, 0]) - np.sort(grid)).max() > 0.002
    # without the option nothing changes
    tf.transcribe2midi([str(clip)], onset_model, dev, str(tmp_path / 'grid'), onset_threshold=thr_on, frame_threshold=thr_fr, min_frames=2)
    save_midi(str(tmp_path / 'grid.mid'), np.array([midi_to_hz(21 + q) for q in p_est]), np.asarray(i_est) * (512 / 16000), [127] * len(p_est))
    assert np.array_equal(parse_midi(str(tmp_path / 'grid' / 'ReconVAT-clip.mid')), parse_midi(str(tmp_path / 'grid.mid')))


def test_evaluate_timing(dev, onset_model):
    from reconvat_amd import evaluate as ev
    from reconvat_amd.dataset import RenderedScores
    from reconvat_amd.decoding import NoteDecoder
    data = RenderedScores(2, 256 * 512, ('struck',), seed=70, device=dev)
    assert min(len(s) for s in data.scores) > 5
    _, _, thr_on, thr_fr = fixture_thresholds(onset_model, data[0]['audio'])
    decoder = NoteDecoder(thr_on, thr_fr, 'rule2', min_frames=2)
    keys = {f'metric/timing/{k}@{t}' for k in ('precision', 'recall', 'f1') for t in ('50ms', '10ms')}
    keys |= {'metric/timing/onset_error_mean_ms', 'metric/timing/onset_error_median_ms'}
    results = {}
    for refine in (False, True):
        with torch.no_grad():
            host = ev.evaluate_timing(data, onset_model, decoder, refine=refine, lead=0, device_metrics=False)
            device = ev.evaluate_timing(data, onset_model, decoder, refine=refine, lead=0, device_metrics=True)
        assert set(host) == set(device) == keys
        for k in keys:
            assert len(host[k]) == 2 and host[k] == device[k], (refine, k)
            assert all(v >= 0 for v in host[k])
        results[refine] = host
    assert all(a <= b + 1e-12 for a, b in zip(results[False]['metric/timing/recall@10ms'], results[False]['metric/timing/recall@50ms']))

    class LabelModel:
        """run_on_batch returns the label rolls: a perfect decoder on the frame grid"""

        def run_on_batch(self, label, *args):
            return {'onset': label['onset'].unsqueeze(0), 'frame': label['frame'].unsqueeze(0)}, {}, None

    grid = ev.evaluate_timing(data, LabelModel(), device_metrics=True)
    fine = ev.evaluate_timing(data, LabelModel(), refine=True, device_metrics=True)
    print('label rolls, grid:', dict(grid), 'refined:', dict(fine))
    for song in range(2):
        assert grid['metric/timing/recall@50ms'][song] == 1.0 and fine['metric/timing/recall@50ms'][song] == 1.0
        assert 0 < fine['metric/timing/onset_error_mean_ms'][song] < grid['metric/timing/onset_error_mean_ms'][song] <= 16.0
        assert fine['metric/timing/f1@10ms'][song] > grid['metric/timing/f1@10ms'][song]
    with torch.no_grad():
        default = ev.evaluate_timing(data, onset_model)                                      # rule2 at 0.5 / 0.5, no refinement
    assert set(default) == keys
    # a dataset without exact note lists, or one that crops its tracks, is refused
    with pytest.raises(ValueError, match='exact note lists'):
        ev.evaluate_timing([data[0]], onset_model)
    cropped = RenderedScores(1, 256 * 512, ('struck',), seed=70, device=dev, sequence_length=64 * 512)
    with pytest.raises(ValueError, match='whole tracks'):
        ev.evaluate_timing(cropped, onset_model)
