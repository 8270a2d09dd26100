"""GPU: the two schedules of the one-pass MMD pair kernel (csrc/gda_mmd_fused.inc) give the same bits.

PYGDA_AMD_MMD_FUSED_SCHED is read once per process, so each schedule runs in a fresh child process of its own (this
file run as a script) over the same shapes and inputs and prints a digest of every output: the loss, the bandwidths,
the partial row gradients ``part`` and, for the gathered path, the gathered rows.  The default schedule runs every
shape twice and also replays it from a captured graph."""
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one-tile segments, odd njb (no partner work item in a workgroup), dead column waves (jt >= ntiles), a tile that holds
# rows of both domains (n % 32 != 0), one segment per resample (n = 7000)
WIDTHS, TIMES, ROWS = (32, 64, 96, 128), (1, 3, 5), (1, 17, 48, 100, 1000, 1001, 7000)


def _digest(*tensors):
    h = hashlib.sha256()
    for x in tensors:
        h.update(x.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _cases():
    return [(d, times, n, gathered) for d in WIDTHS for times in TIMES for n in ROWS for gathered in (False, True)]


def _run(d, times, n, gathered, graph=False):
    from pygda_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(7919 * d + 131 * times + n + (1 << 20) * gathered)
    if gathered:
        ns, nt = n + 37, 2 * n + 5
        s = torch.randn(ns, d, generator=gen).relu().to(dev)
        t = (torch.randn(nt, d, generator=gen) * 1.3 + 0.2).relu().to(dev)
        si = torch.randint(0, ns, (times, n), generator=gen).to(dev)
        ti = torch.randint(0, nt, (times, n), generator=gen).to(dev)
        rs = torch.empty(times * n, d, device=dev)
        rt = torch.empty(times * n, d, device=dev)
    else:
        s = torch.randn(times * n, d, generator=gen).to(dev)
        t = (torch.randn(times * n, d, generator=gen) * 0.8 + 0.3).to(dev)
        si = ti = rs = rt = None
    nseg = L.gda_mmd_fused_nseg(times, n, d, 2.0, 5)
    assert nseg > 0
    m = 2 * n
    loss = torch.empty(1, device=dev)
    bw = torch.empty(times, device=dev)
    part = torch.empty(times, nseg, m, d, device=dev)
    ws = torch.zeros(L.gda_mmd_workspace_bytes(times, n, d), dtype=torch.uint8, device=dev)

    def call():
        _lib.check(L.gda_mmd_fused_fwd_f32(
            _lib.ptr(s), d, _lib.ptr(t), d, d, _lib.ptr(si), _lib.ptr(ti), times, n, 2.0, 5, 0.0, 1.0, None,
            _lib.ptr(rs), _lib.ptr(rt), _lib.ptr(loss), _lib.ptr(bw), _lib.ptr(part), nseg, _lib.ptr(ws), ws.numel(),
            _lib.stream()), "gda_mmd_fused_fwd_f32")

    outs = lambda: (loss, bw, part) + ((rs, rt) if gathered else ())
    call()
    torch.cuda.synchronize()
    first = _digest(*outs())
    if not graph:
        return first, None, None
    call()
    torch.cuda.synchronize()
    again = _digest(*outs())
    for x in outs():
        x.fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    g.replay()
    torch.cuda.synchronize()
    replayed = _digest(*outs())
    del g
    return first, again, replayed


def _child(sched):
    env = dict(os.environ, PYGDA_AMD_MMD_FUSED_SCHED=str(sched))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(sched)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_mmd_pair_kernel_schedules_give_the_same_bits():
    old, new = _child(0), _child(1)
    assert len(old) == len(new) == len(_cases())
    for case, (o, _, _), (a, b, c) in zip(_cases(), old, new):
        assert a == o, f"schedules differ at (d, times, n, gathered) = {case}"
        assert b == a, f"two calls of the default schedule differ at {case}"
        assert c == a, f"the captured replay differs from the eager call at {case}"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sched = int(sys.argv[1])
    print(json.dumps([list(_run(*case, graph=sched != 0)) for case in _cases()]))
