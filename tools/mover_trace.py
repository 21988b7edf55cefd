"""Per-iteration view of the headline run (sample start, lazy statistics) with the mover tile off and on, alternating in one
process on one dataset: the assignment stage's time (both screen launches and k_certify_movers lie inside the first timing
pair), the whole iteration's wall time, the form, the steps settled by the carried bounds and the mover tile's three counters
(steps that passed test B only / certified on the tile / sent on).  With the form off the first counter is the share that
DESIGN section 4.4's model assumes.  A second row per iteration holds the second level's counters (steps that passed test
B2 only / certified on the two tiles / sent on).  level = 2: the SECOND level is what alternates, the first stays on.
usage: python tools/mover_trace.py [n] [iterations] [repeats] [order] [level]"""
import os, sys, time, ctypes as C, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparsifiedkmeans_amd import _lib, synth
from sparsifiedkmeans_amd.engine import LloydEngine, Shard, torch_context, mix_device
ctx = torch_context(0)
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100_000_000
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 14
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 2
order = sys.argv[4] if len(sys.argv) > 4 else "block"
level = int(sys.argv[5]) if len(sys.argv) > 5 else 1
name = "mover_tile" if level == 1 else "mover_tiles2"
K, p = 100, 1024
d = synth.sparsified_gmm_device(ctx, p, n, n, 0, K, 0.05, seed=234, order=order)
sh = Shard.from_device(ctx, d["p2"], d["jc"], d["ir"], d["x"], nnz=d["nnz"])
sh.set_lazy_stats(True)
g = torch.Generator(device="cuda"); g.manual_seed(234 + 17)
lab = torch.randint(0, K, (K,), generator=g, device="cuda")
start = d["means"][lab] + 0.1 * torch.randn((K, p), generator=g, device="cuda", dtype=torch.float64)
c0 = mix_device(ctx, start.contiguous(), d["p2"], d["sign"], 1.0, float(np.sqrt(np.float64(d["p2"]))))
L = _lib.lib()
steps = (n + 15) // 16
totals = {}
for rep in range(repeats):
    for on in (False, True):
        for v in ("SPKM_MOVER_TILE", "SPKM_NO_MOVER_TILE", "SPKM_MOVER_TILE2", "SPKM_NO_MOVER_TILE2"):
            os.environ.pop(v, None)
        if level == 1:
            os.environ["SPKM_MOVER_TILE" if on else "SPKM_NO_MOVER_TILE"] = "1"
            os.environ["SPKM_NO_MOVER_TILE2"] = "1"
        else:
            os.environ["SPKM_MOVER_TILE"] = "1"
            os.environ["SPKM_MOVER_TILE2" if on else "SPKM_NO_MOVER_TILE2"] = "1"
        ctx.reload_switches()
        sh.reset_policy()
        eng = LloydEngine(sh, K, d["gamma"])
        c = c0.clone()
        scr, wall = [], []
        for it in range(iters):
            _lib.check(L.spkm_timing_log(ctx.handle, 2))
            torch.cuda.synchronize(); t0 = time.perf_counter()
            eng.iterate(c, want_mind=False)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            buf = (C.c_double * 4)(); cnt = C.c_int()
            _lib.check(L.spkm_timing_read(ctx.handle, buf, 4, C.byref(cnt)))
            m, ms, ms2 = eng.last_screen_mode(), eng.last_mover_steps(), eng.last_mover_steps2()
            scr.append(buf[0]); wall.append(dt * 1e3)
            print(f"{name}={'on ' if on else 'off'} run {rep} iter {it + 1:2d}: {dt * 1e3:6.2f} ms  screen {buf[0]:6.2f}  form {m[0]} listed {m[1]} "
                  f"early {m[3]} skipped {m[4] / steps:.3f}  B-only {ms[0] / steps:.3f} certified {ms[1] / steps:.3f} sent on {ms[2] / steps:.3f}", flush=True)
            print(f"{name}={'on ' if on else 'off'} run {rep} iter {it + 1:2d}:   second level  B2-only {ms2[0] / steps:.3f} certified {ms2[1] / steps:.3f} "
                  f"sent on {ms2[2] / steps:.3f}", flush=True)
        _lib.check(L.spkm_timing_log(ctx.handle, 0))
        totals.setdefault(on, []).append((sum(scr), sum(wall)))
        print(f"{name}={'on ' if on else 'off'} run {rep}: screen stage {sum(scr):.2f} ms, wall {sum(wall):.2f} ms over {iters} iterations; "
              f"final centres checksum {float(c.abs().sum()):.12e}", flush=True)
for on, v in totals.items():
    print(name, "on " if on else "off", "screen-stage totals", [round(a, 2) for a, _ in v], "wall totals", [round(b, 2) for _, b in v])
