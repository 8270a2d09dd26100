#!/usr/bin/env python
"""Where does a workgroup of the register-resident one-pass MMD (k_mmd_fused / k_mmd_fused_pp) spend its time?  Needs a
tracing build of gda_mmd.hip:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -DGDA_MMD_TRACE -shared pygda_amd/csrc/gda_mmd.hip -o <lib.so>
    PYGDA_AMD_MMD_FUSED_SCHED=0|1 python tools/mmd_fused_trace.py <lib.so> [d, default 128] [resamples, default 5]

Calls gda_mmd_fused_fwd_f32 at (resamples, 1000 rows per domain, d) a few times and prints, from the clock stamps of the
last call (s_memtime, lane 0 of wave 0 and of wave 4 -- the two waves of SIMD 0 -- in every workgroup), the mean cycles
per workgroup of: the prologue (column operands, bandwidth fold, first images), per tile the distance product S, the
exponentials E and the gradient product O, the gaps between them (the barrier and its waits sit in one of them), the
tail (reduction, result), and how far the two waves of a SIMD are apart (start of S on wave 4 minus on wave 0)."""
import ctypes
import os
import sys

import torch

P = ctypes.c_void_p
TILES = 16
SLOT = 2 + 6 * TILES + 2                      # FZ_TR_SLOT in csrc/gda_mmd_fused.inc


def main():
    lib = ctypes.CDLL(sys.argv[1])
    d = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    times, n = (int(sys.argv[3]) if len(sys.argv) > 3 else 5), 1000
    pp = os.environ.get("PYGDA_AMD_MMD_FUSED_SCHED", "1")[:1] != "0"
    dev = torch.device("cuda:0")
    lay = (ctypes.c_int64 * 16)()
    assert lib.gda_mmd_fused_layout(times, ctypes.c_int64(n), ctypes.c_int64(d), lay, 16) == 0
    nb, ntiles, njb, nseg, total = list(lay)[:5]
    nwg = times * nseg * ((njb + 1) // 2) if pp else total
    print(f"d {d}: schedule {'pp (8 waves, two work items)' if pp else 'one item (4 waves)'}: ntiles {ntiles} njb {njb} "
          f"nseg {nseg} workgroups {nwg}")
    lib.gda_mmd_workspace_bytes.restype = ctypes.c_size_t
    wsb = lib.gda_mmd_workspace_bytes(times, ctypes.c_int64(n), ctypes.c_int64(d))
    gen = torch.Generator().manual_seed(1)
    s = torch.randn(times * n, d, generator=gen).relu().to(dev)
    t = (torch.randn(times * n, d, generator=gen) * 1.3 + 0.2).relu().to(dev)
    part = torch.empty(times, nseg, 2 * n, d, device=dev)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    loss, bw = torch.empty(1, device=dev), torch.empty(times, device=dev)
    trace = torch.zeros((total + 8) * 2 * SLOT, dtype=torch.int64, device=dev)
    assert lib.gda_dbg_mmd_trace(P(trace.data_ptr())) == 0
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(5):
        st = lib.gda_mmd_fused_fwd_f32(
            P(s.data_ptr()), ctypes.c_int64(d), P(t.data_ptr()), ctypes.c_int64(d), ctypes.c_int64(d), None, None, times,
            ctypes.c_int64(n), ctypes.c_float(2.0), 5, ctypes.c_float(0.0), ctypes.c_float(1.0), None, None, None,
            P(loss.data_ptr()), P(bw.data_ptr()), P(part.data_ptr()), int(nseg), P(ws.data_ptr()), ctypes.c_size_t(wsb),
            P(stream))
        assert st == 0, st
    torch.cuda.synchronize()
    tr = trace.view(-1, 2, SLOT)[:nwg].cpu().double()
    ntile = [int(seg + 1) * ntiles // nseg - int(seg) * ntiles // nseg for seg in range(nseg)]
    lmin = min(min(ntile), TILES)
    wav = [0, 1] if pp else [0]
    t0 = tr[:, 0, 0].min()
    for h in wav:
        x = tr[:, h]
        ok = x[:, 0] > 0
        x = x[ok]
        ts = lambda k, i: x[:, 2 + 6 * k + i]
        print(f" wave {4 * h} ({int(ok.sum())} workgroups; per tile: the first {lmin} tiles of every segment)")
        print(f"  prologue {float((x[:, 1] - x[:, 0]).mean()):8.0f}")
        seg = {"S": [], "S->E": [], "E": [], "E->O": [], "O": [], "O->S": []}
        for k in range(lmin):
            seg["S"].append(ts(k, 1) - ts(k, 0)); seg["S->E"].append(ts(k, 2) - ts(k, 1))
            seg["E"].append(ts(k, 3) - ts(k, 2)); seg["E->O"].append(ts(k, 4) - ts(k, 3))
            seg["O"].append(ts(k, 5) - ts(k, 4))
            if k + 1 < lmin:
                seg["O->S"].append(ts(k + 1, 0) - ts(k, 5))
        for nm, v in seg.items():
            if v:
                v = torch.stack(v)
                print(f"  {nm:5s} mean {float(v.mean()):7.0f}  per tile " + " ".join(f"{float(c):6.0f}" for c in v.mean(1)))
        step = (ts(lmin - 1, 0) - ts(0, 0)) / max(lmin - 1, 1)
        print(f"  per tile (start of S to start of S) {float(step.mean()):8.0f}")
        print(f"  loop end -> end (tail) {float((x[:, SLOT - 1] - x[:, SLOT - 2]).mean()):8.0f}   "
              f"whole workgroup {float((x[:, SLOT - 1] - x[:, 0]).mean()):8.0f}")
    if pp:
        both = (tr[:, 0, 0] > 0) & (tr[:, 1, 0] > 0)
        lag = [tr[both, 1, 2 + 6 * k] - tr[both, 0, 2 + 6 * k] for k in range(lmin)]
        print("  wave 4 behind wave 0 at the start of S, per tile: " + " ".join(f"{float(v.mean()):6.0f}" for v in lag))
    ends = tr[:, :, SLOT - 1].max(1).values
    print(f"  kernel span {float(ends.max() - t0):9.0f} ticks; starts spread {float(tr[:, 0, 0].max() - t0):7.0f}")
    print("  loss", float(loss))


if __name__ == "__main__":
    main()
