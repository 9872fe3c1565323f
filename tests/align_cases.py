"""Shared cases of tests/test_align.py and tests/test_align_gpu.py: the plain double loop the yardstick is checked against, the
rendered score / recording pair of the end-to-end tests, the hand-made band and the folder of the CLI tests."""
import os

import numpy as np
import torch

from reconvat_amd import align, synth

INF = align.SENTINEL


def dtw_loop(cost, lo, W, M):
    """The definition as a plain double loop over the cells of the band: (total, dirs [N][W], D as a dict)."""
    N = len(lo)
    D, dirs = {}, np.full((N, W), 3, dtype=np.uint8)
    for i in range(N):
        for j in range(int(lo[i]), min(int(lo[i]) + W, M)):
            c = int(cost[i, j - lo[i]])
            if i == 0 and j == 0:
                D[i, j] = 2 * c
                continue
            best, code = INF, 3
            for k, (pi, pj, w) in enumerate(((i - 1, j - 1, 2), (i - 1, j, 1), (i, j - 1, 1))):
                v = D.get((pi, pj), INF)
                if v != INF and v + w * c < best:
                    best, code = v + w * c, k
            D[i, j] = best
            dirs[i, j - lo[i]] = code
    return D.get((N - 1, M - 1), INF), dirs, D


def path_loop(dirs, lo, N, M):
    """The path as a list of cells, walked back from the corner."""
    i, j, cells = N - 1, M - 1, []
    while True:
        cells.append((i, j))
        if i == 0 and j == 0:
            return cells[::-1]
        code = dirs[i, j - lo[i]]
        i, j = i - (code != 2), j - (code != 1)


def check_result(res, cost, lo, W, M):
    """A result dict (yardstick or device) against the double loop: total, length, the four arrays, the directions of reachable cells."""
    N = len(lo)
    total, dirs, D = dtw_loop(cost, lo, W, M)
    assert res['total'] == total
    if total == INF:
        assert res['length'] == 0
        for key, n in (('row_lo', N), ('row_hi', N), ('col_lo', M), ('col_hi', M)):
            assert (res[key] == -1).all() and len(res[key]) == n
    else:
        cells = path_loop(dirs, lo, N, M)
        assert res['length'] == len(cells)
        for key, axis, other, pick, n in (('row_lo', 0, 1, min, N), ('row_hi', 0, 1, max, N), ('col_lo', 1, 0, min, M), ('col_hi', 1, 0, max, M)):
            want = [pick(c[other] for c in cells if c[axis] == v) for v in range(n)]
            assert res[key].tolist() == want, key
    if 'dirs' in res:
        reach = np.zeros(dirs.shape, dtype=bool)
        for (i, j), v in D.items():
            reach[i, j - lo[i]] = v != INF
        assert (res['dirs'][reach] == dirs[reach]).all()


def same_result(a, b, dirs_where=None):
    for key in ('total', 'length'):
        assert a[key] == b[key], (key, a[key], b[key])
    for key in ('row_lo', 'row_hi', 'col_lo', 'col_hi'):
        assert np.array_equal(a[key], b[key]), key
    if dirs_where is not None:
        assert np.array_equal(a['dirs'][dirs_where], b['dirs'][dirs_where])


def reachable(res_host, cost):
    """Cells whose direction byte is defined: live and reachable (the yardstick leaves 3 everywhere else; the start cell holds 3 too)."""
    return (np.asarray(cost) != align.DEAD) & (res_host['dirs'] != 3)


def jumpy_lo(N=70, M=200, W=33):
    """A hand-made band: plateaus, jumps of 1, of 31 and of W - 1, and rows whose band is cut off at M."""
    steps = [0] * 10 + [1] * 8 + [0] * 5 + [31] + [0] * 6 + [1] * 4 + [W - 1] + [0] * 3 + [31] + [1] * 10 + [0] * 4 + [W - 1] + [0] * 2 + [1] * 5 + [31] + [1] * 4
    steps = (steps + [0] * N)[:N - 1]
    lo = np.concatenate([[0], np.cumsum(steps)])
    assert lo[-1] + W > M > lo[-1] and len(lo) == N                # the last rows are cut off at M and still reach column M - 1
    return lo.astype(np.int32)


def unit_rows(rng, n, D):
    """Non-negative unit rows with a shared component, so that costs spread over (0, 1) instead of crowding at 1."""
    x = rng.rand(n, D) ** 4 + 0.05
    return x / np.sqrt((x * x).sum(1, keepdims=True))


# ---- the end-to-end case: a 12 s random score, rendered plainly as "the score" and, warped, in another timbre, with noise, as "the recording"
SECONDS, SEED = 12.0, 3
warp = lambda t: 0.4 + 1.15 * t + 0.5 * np.sin(2.0 * np.pi * t / 7.0)
_CASE = {}


def warped_notes(notes):
    out = np.array(notes, dtype=np.float64)
    out[:, 0], out[:, 1] = warp(out[:, 0]), warp(out[:, 1])
    return out


def recording_of(notes, timbre, noise_seed, amplitude=5e-4):
    """The warped notes rendered on the host with white noise added (default -66 dBFS: above that the noise outweighs KAPPA in the
    leading silence and the first onsets go astray, DESIGN 3.16 has the table): int16 [n]."""
    w = warped_notes(notes)
    n = align.score_length(w)
    y = synth.render_host(synth.partials(w, timbre), 0, n)
    y = y + amplitude * np.random.RandomState(noise_seed).randn(n)
    return synth.to_int16(y)


def e2e_case():
    """(score notes, recording int16, true onsets in the recording), built once."""
    if not _CASE:
        notes = synth.random_score(np.random.RandomState(SEED), SECONDS)
        _CASE['v'] = (notes, recording_of(notes, synth.Timbre('struck', 7), 5), warp(notes[:, 0]))
    return _CASE['v']


def onset_share(aligned, truth, tol=0.05):
    return float((np.abs(aligned[:, 0] - truth) <= tol).mean())


def make_folder(folder, n=6, seconds=6.0):
    """n short rendered recordings name.wav; all but the last with a score in SCORE time beside them (.score.tsv, every other one .mid).
    Returns the score notes per name."""
    from scipy.io import wavfile
    from reconvat_amd.midi import parse_midi
    scores = {}
    for i in range(n):
        name = f'piece{i}'
        notes = synth.random_score(np.random.RandomState(100 + i), seconds)
        wavfile.write(os.path.join(folder, name + '.wav'), 16000, recording_of(notes, synth.Timbre('struck', 20 + i), 50 + i))
        if i == n - 1:
            continue
        if i % 2:
            write_midi(os.path.join(folder, name + '.mid'), notes)
            notes = np.asarray(parse_midi(os.path.join(folder, name + '.mid')), dtype=np.float64).reshape(-1, 4)
        else:
            align.write_tsv(os.path.join(folder, name + '.score.tsv'), notes)
            notes = align.read_score(os.path.join(folder, name + '.score.tsv'))
        scores[name] = notes
    return scores


def _vlq(v):
    out = [v & 0x7F]
    v >>= 7
    while v:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    return bytes(out[::-1])


def write_midi(path, notes, tpq=480, tempo=500000):
    """A minimal format-0 MIDI file of tsv rows (one track, one tempo)."""
    tick = lambda t: int(round(t * 1e6 / tempo * tpq))
    events = []
    for on, off, m, v in np.asarray(notes, dtype=np.float64).reshape(-1, 4):
        events.append((tick(on), 1, bytes([0x90, int(m), int(v)])))
        events.append((max(tick(off), tick(on) + 1), 0, bytes([0x80, int(m), 0])))
    events.sort(key=lambda e: (e[0], e[1]))
    body, now = b'\x00\xff\x51\x03' + tempo.to_bytes(3, 'big'), 0
    for t, _, msg in events:
        body += _vlq(t - now) + msg
        now = t
    body += b'\x00\xff\x2f\x00'
    with open(path, 'wb') as fh:
        fh.write(b'MThd' + (6).to_bytes(4, 'big') + (0).to_bytes(2, 'big') + (1).to_bytes(2, 'big') + tpq.to_bytes(2, 'big'))
        fh.write(b'MTrk' + len(body).to_bytes(4, 'big') + body)
