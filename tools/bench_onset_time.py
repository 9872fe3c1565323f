"""The onset refiner (rv_onset_refine; profiles/onset_time.txt keeps the output) on the notes of a rendered ten-minute track
('struck', seed 1, true keys, the frames of a perfect decoder), next to

    numpy       the definition (onset_time.refine_host, float64) on the host, one run
    torch       the same product composed from torch ops on the same device: the 2048-sample windows gathered, `unfold(512, 32)` into
                [n, 49, 512] and one batched `matmul` with the keys' [512, 16] table slices, then the root, the differences, argmax
                and the median by sort

Times are HIP-event times around one call, warm, the median of REPS windows of INNER calls (min and max beside it).  Before any time is
printed the kernel's samples are compared with the host's (the share of equal notes is printed: the two differ where float32 decides a
near-tie) and with the vote on its own amplitudes (equal on every note), and the torch composition with the kernel.  512 MFMAs
(v_mfma_f32_16x16x4_f32, 32 cycles each) per note is the arithmetic the time is set against."""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from reconvat_amd import _lib, onset_time as ot, synth

REPS, INNER = 21, 10
SECONDS, SEED = 600, 1

if not torch.cuda.is_available():
    raise SystemExit('bench_onset_time.py measures on the GPU; there is none')
dev = torch.device('cuda:0')
torch.cuda.set_device(dev)


def timed(fn):
    for _ in range(INNER):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / INNER)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


notes = synth.random_score(np.random.RandomState(SEED), float(SECONDS))
audio = synth.render(notes, SECONDS * 16000, synth.Timbre('struck', SEED), device=dev, out_dtype=torch.int16).float().div(32768.0)
keys = notes[:, 2].astype(np.int64) - 21
frames = np.rint(notes[:, 0] * 16000 / 512).astype(np.int64)
n, T = len(keys), audio.numel()

# ---- the kernel, as the package calls it (the notes are uploaded per call) and with the notes resident
table = ot.device_table(dev)
d_notes = torch.from_numpy(np.stack([keys, frames], axis=1).astype(np.int32)).to(dev)
d_out = torch.empty(n, dtype=torch.int32, device=dev)


def kernel():
    _lib.call('rv_onset_refine', audio.data_ptr(), T, table.data_ptr(), d_notes.data_ptr(), n, 0, d_out.data_ptr(), None, _lib.stream())


# ---- the torch composition
d_keys, d_frames = torch.from_numpy(keys).to(dev), torch.from_numpy(frames).to(dev)
B = table.reshape(88, 16, 512).transpose(1, 2).contiguous()                                  # [88, 512, 16]
V = torch.from_numpy(ot.valid_harmonics()).to(dev)


def composed():
    idx = (512 * d_frames - 1024)[:, None] + torch.arange(2048, device=dev)[None, :]
    inside = (idx >= 0) & (idx < T)
    win = torch.where(inside, audio[idx.clamp(0, T - 1)], torch.zeros((), device=dev))
    D = torch.matmul(win.unfold(1, 512, 32), B[d_keys])                                      # [n, 49, 16]
    A = D.reshape(n, 49, 8, 2).square().sum(-1).sqrt()
    kq = (A[:, 2:] - A[:, :-2]).argmax(dim=1) + 1
    valid = torch.arange(8, device=dev)[None, :] < V[d_keys][:, None]
    kq = torch.where(valid, kq, torch.full_like(kq, 49)).sort(dim=1).values
    k = kq.gather(1, ((V[d_keys] - 1) // 2)[:, None]).reshape(-1)
    return (512 * d_frames - 768 + 32 * k).clamp(0, T - 1)


host_audio = audio.cpu().numpy()
t0 = time.perf_counter()
want = ot.refine_host(host_audio, keys, frames)
numpy_s = time.perf_counter() - t0
got, amp = ot.refine_device(audio, keys, frames, return_amplitudes=True)
got, amp = got.cpu().numpy().astype(np.int64), amp.cpu().numpy()
assert np.array_equal(got, ot._samples(ot.pick(amp, keys), frames, 0, T))
kernel()
torch.cuda.synchronize()
assert np.array_equal(d_out.cpu().numpy(), got)
torch_out = composed().cpu().numpy()
result = {'notes': n, 'samples': T, 'equal_to_host': float(np.mean(got == want)), 'torch_equal_to_kernel': float(np.mean(torch_out == got)),
          'error_ms_grid': float(np.mean(np.abs(frames * 512 / 16000 - notes[:, 0])) * 1e3),
          'error_ms_refined': float(np.mean(np.abs(got / 16000 - notes[:, 0])) * 1e3), 'numpy_s': numpy_s}
k = timed(kernel)
p = timed(lambda: ot.refine_device(audio, keys, frames))
e = timed(composed)
result.update(kernel_us=k[0], kernel_us_min_max=k[1:], package_call_us=p[0], package_call_us_min_max=p[1:], torch_us=e[0],
              torch_us_min_max=e[1:], torch_over_kernel=e[0] / k[0], numpy_over_kernel=numpy_s * 1e6 / k[0],
              ns_per_note=k[0] * 1e3 / n, mfma_per_note=512, mfma_cycles_per_note=512 * 32)
print(f"{n} notes of a {SECONDS} s track: kernel {k[0]:.1f} us ({result['ns_per_note']:.0f} ns per note), package call {p[0]:.1f} us, "
      f"torch ops {e[0]:.1f} us, numpy {numpy_s * 1e3:.0f} ms; equal to the host on {100 * result['equal_to_host']:.1f} % of the notes; "
      f"onset error {result['error_ms_grid']:.2f} -> {result['error_ms_refined']:.2f} ms")
print(json.dumps(result))
