"""GPU box: the event pass of a far shard with incremental sums (spkm_shard_set_far_events) against the full accumulation pass,
at chosen shares of movers -- the measurement behind the mover bar of the far branch in csrc/policy.h
(profiles/far_events_ab.txt).  Teacher-forced: a planted mixture at d = 8192, s = 82, K = 100 whose clusters 0 and 1 hold
0.5 % of the points each and the others 1 % each; exchanging the centres of a set of clusters between calls moves exactly
their members.  Per share: the kernel time of the accumulation stage (the second HIP-event pair of spkm_timing_log(ctx, 2))
of a call that applies the movers' events one by one (its predecessor counted no mover), of calls that sort them and add
them up in slabs (its predecessor counted as many), and of the same calls under SPKM_NO_INCREMENTAL=1 (the full pass).
    python tools/far_events_bar.py [N]"""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from sparsifiedkmeans_amd import _lib                                    # noqa: E402
from sparsifiedkmeans_amd.engine import LloydEngine, Shard, torch_context  # noqa: E402

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
p, s, K = 8192, 82, 100
dev = "cuda:0"
ctx = torch_context(0)
L = _lib.lib()
g = torch.Generator(device=dev)
g.manual_seed(7)
prob = torch.full((K,), 0.99 / (K - 2), device=dev, dtype=torch.float64)
prob[:2] = 0.005
labels = torch.multinomial(prob, n, replacement=True, generator=g)
centres = torch.randn((K, p), generator=g, device=dev, dtype=torch.float64)
ir = torch.empty(n * s + 48, dtype=torch.int16, device=dev)
x = torch.zeros(n * s + 48, dtype=torch.float64, device=dev)
ir[n * s:] = 0
CH = 500_000
for a in range(0, n, CH):                                   # s distinct rows per point, ascending; value = its centre + noise
    b = min(n, a + CH)
    r0 = torch.randint(0, p, (b - a, 1), generator=g, device=dev)
    step = 1 + 2 * torch.randint(0, 49, (b - a, 1), generator=g, device=dev)
    rows = torch.sort((r0 + step * torch.arange(s, device=dev)[None, :]) % p, dim=1).values
    v = centres[labels[a:b, None], rows] + 1.0 * torch.randn((b - a, s), generator=g, device=dev, dtype=torch.float64)
    ir[a * s:b * s] = rows.reshape(-1).to(torch.int16)                     # (rows < 8192)
    x[a * s:b * s] = v.reshape(-1)
    del rows, v, r0, step
jc = torch.arange(0, (n + 1) * s, s, dtype=torch.int64, device=dev)
shard = Shard.from_device(ctx, p, jc, ir, x, nnz=n * s)
gam = s / p
for f in (shard.set_far_screen, shard.set_far_bounds, shard.set_sliced_sums, shard.set_far_events, shard.set_lazy_stats):
    f(True)
eng = LloydEngine(shard, K, gam)
base = (gam * centres).contiguous()


def swapped(ks):
    c = base.clone()
    c[ks] = base[ks[1:] + ks[:1]]
    return c.contiguous()


def acc_ms(c):
    _lib.check(L.spkm_timing_log(ctx.handle, 2))
    eng.assign_accumulate_step(c, want_mind=False)
    torch.cuda.synchronize()
    buf, cnt = (C.c_double * 8)(), C.c_int()
    _lib.check(L.spkm_timing_read(ctx.handle, buf, 8, C.byref(cnt)))
    _lib.check(L.spkm_timing_log(ctx.handle, 0))
    return buf[1], eng.last_screen_mode()[6]


def movers(prev):
    a = eng.assign.clone()
    return a, int((a != prev).sum().item())


print(f"n = {n}, p = {p}, s = {s}, K = {K}")
for name, ks in (("1 %", [0, 1]), ("10 %", list(range(2, 12))), ("20 %", list(range(2, 22))), ("32 %", list(range(2, 34))),
                 ("33.4 %: past the bar", list(range(2, 35)))):
    other = swapped(ks)
    rows = {}
    for mode in ("events", "full"):
        if mode == "full":
            os.environ["SPKM_NO_INCREMENTAL"] = "1"
        else:
            os.environ.pop("SPKM_NO_INCREMENTAL", None)
        ctx.reload_switches()
        shard.reset_policy()
        acc_ms(base)                                        # no bounds yet: the full pass
        prev, _ = movers(eng.assign)
        acc_ms(base)                                        # counted: no mover
        t = []
        for c in (other, base, other):                      # one by one (after a count of 0), then sorted twice
            ms, form = acc_ms(c)
            prev, m = movers(prev)
            t.append((round(ms, 3), form, m))
        rows[mode] = t
    print(f"movers {name}: events {rows['events']}   full pass {rows['full']}   (ms, info[6], movers)")
os.environ.pop("SPKM_NO_INCREMENTAL", None)
