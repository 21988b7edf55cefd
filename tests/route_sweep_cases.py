"""Drawn cases of tests/test_gpu_route_sweep.py and of the CPU test that keeps it from passing vacuously
(tests/test_route_sweep_cases_cpu.py): short Lloyd runs on DRAWN shapes over every opt-in screen route of the fused call and the
opt-ins that stack on them (csrc/policy.h), disturbed mid-way as the driver's EmptyAction disturbs a run, and followed by a second
run at another K on the same shard.  No GPU, no torch, nothing of the library: numpy, tests/util.random_csc and the oracle; the
route a case takes is predicted through the plan harnesses (tests/plan_harness.py and the two small ones beside it).

  draw(route, seed)   a case: shapes, data recipe, opt-ins, the disturbance and the second run's K -- a dict of plain values
  data(case)          (X, gamma, C0, C2): the shard, the centres the first run starts from, those of the second run
  replay(case, o)     a generator over the calls of the script, stepping the oracle: what every call must return
  route_of(...)       the route and tile / plane width the fused call takes, by the library's own plan functions

THE DATA are the planted shards of test_gpu_sweeps._lloyd_run_random_shape -- random_csc, 0.3 x its values + the planted centre's
entry, C0 = gamma cen0 + 0.05 noise, a duplicate centre on every third seed -- with ONE change: every stored value is rounded to a
multiple of 1/8 and clipped to +-64.  A per-cluster, per-row sum of up to 4096 such values is a multiple of 1/8 below 2^18: 22
significand bits, exact in f64 in any order and under any history of additions and subtractions.  So sums, counts and cluster sizes
are compared BIT FOR BIT on every route, the event routes included, and there is no tolerance to choose.

Two conditions on the draws, both for the sake of the policy's cool-down (more than 5 % of the points on the exact list: 8 calls on
the all-exact kernels, csrc/policy.h spkm_policy::observe):
  * the duplicate centre ties every member of its cluster for good (the second copy stays empty, so its column is never updated):
    n / K points that no screen certifies, in every call.  It is drawn only where K >= 32 and n >= 200: at most 3.2 % of the points;
  * where n is one of the small values a single listed point is more than 5 %: no duplicate there.

THE SCRIPT of a case, 0-based calls:
  0 .. 5      Lloyd iterations, each on the centres the update of the call before produced;
  at T in {1, 2, 3}   ONE disturbance of the centres going in:
     (largest: by the members that store an entry; never centroid 0 of a shard with empty columns, which keeps them)
     'swap'   the two largest clusters of call T - 1 exchange their centres: every member of both moves;
     'far'    the centre of the largest cluster of call T - 1 := 40 max|C| in every row: its cluster empties in call T, and call
              T + 1 follows up as the driver does one call after an empty cluster --
              'singleton'  the emptied centre := the stored column of the point farthest from its centre in call T, first index
                           (kmeans_sparsified.m:436-437; divided by gamma in the distance, it loses that point again);
              'drop'       the emptied centre is removed: K - 1 centres, and the caller builds a NEW engine on the same shard
                           WITHOUT reset_policy, as sparsifiedkmeans_amd/kmeans.py does;
  6, 7 (, 8)  the centres of call 5 again, unchanged: zero drift.  (8: only with incremental sums, whose calls alternate lazy /
              with distances -- a second lazy repeat, should the first not be allowed its events);
  then        reset_policy() and a SECOND RUN of 3 iterations at K2 -- drawn from the route's whole range, so it may exceed K (on
              every fourth seed it is made to); on every fourth seed K2 = the K the first run ended on, and the run keeps the
              first one's ENGINE: the one case in which bounds that reset_policy failed to drop would be believed (another K, or
              a new assignment buffer, makes the library start over by itself) -- from fresh centres.
With lazy statistics every odd call asks for its distances, every even one does not."""
import functools

import numpy as np

from util import parts, random_csc

LDS160, CUS = 163840, 256
ROUTES = ("quad", "tile", "wide", "far", "far_ragged", "tile_ragged", "many", "none")
# seeds per route: 8, and 10 where the table has five opt-in sets (each has to occur twice)
SEEDS = {"quad": 8, "tile": 10, "wide": 10, "far": 8, "far_ragged": 8, "tile_ragged": 8, "many": 8, "none": 10}
SMALL_N = (1, 15, 17, 63, 65, 1023, 1025)
N_MAX = 3000
UNIT, CLIP = 0.125, 64.0
assert N_MAX <= 4096 and N_MAX * CLIP / UNIT < 2.0 ** 53 and 4096 * CLIP / UNIT <= 2.0 ** 22   # the exactness bound

# the opt-in sets of the table; "lazy" = spkm_shard_set_lazy_stats
TILE_SETS = ((), ("wide_bounds",), ("tile_far",), ("tile_far", "far_bounds"), ("tile_far", "far_bounds", "far_events", "lazy"))
FAR_SETS = (("far_bounds",), ("far_bounds", "far_events", "lazy"), ("sliced_sums",), ("far_bounds", "far_events", "lazy", "sliced_sums"))
PIPE_SETS = (("far_bounds",), ("far_bounds", "far_events", "lazy"))
DISTURBANCES = ("swap", "far+singleton", "far+drop")
K_RANGE = {"quad": (2, 200), "tile": (17, 300), "wide": (2, 256), "far": (2, 300), "far_ragged": (2, 300), "tile_ragged": (2, 300),
           "many": (1025, 2200)}


# ---- the limits at an LDS size, restated in plain integers (the CPU test holds the draws to the library's own functions) ----
def last_p(L, kt):
    """the largest p whose f32 tile of kt centroids -- p + 1 rows of 4 kt bytes and the 16 bytes of the work ticket -- fits"""
    return (L - 16) // (4 * kt) - 1


def s_cap(L, p):
    """the longest column with an exact pass behind a tile: p 20 + 1024 + 16 8 (s | 1) 8 <= L"""
    m = (L - 1024 - 20 * p) // 1024
    return m if m % 2 else m - 1


def _ints(rng, lo, hi):
    return int(rng.integers(lo, hi + 1))


def draw(route, seed):
    """the case (route, seed), deterministic; every limit is the one of 160 KB of LDS and 256 CUs"""
    assert route in ROUTES
    L = LDS160
    rng = np.random.default_rng([ROUTES.index(route), seed, 4242])
    c = dict(route=route, seed=seed, ragged=False, opts=(), no_direct=False, bits=32 if (seed // 2) % 2 else 16)
    shape_of = route
    if route == "none":
        # a shape of another route with that route's own opt-in withheld; the others stay, and must change nothing
        shape_of = ("wide", "far", "far_ragged", "tile_ragged", "many")[seed % 5]
    c["shape_of"] = shape_of
    band = None
    if shape_of == "quad":
        p = int(rng.choice([64, 100, 256, 500, 1024, last_p(L, 32)]))
        s = _ints(rng, 1, min(64, p))
        c["opts"] = ("lazy",) if seed % 2 else ()
        if seed % 4 == 1:
            band = (2, 128)                                    # (pair events, below: K (K + 1) counters in LDS, K <= 128)
    elif shape_of == "tile":
        p = last_p(L, 32) if seed % 5 == 0 else _ints(rng, 128, last_p(L, 32))
        s = _ints(rng, 65, min(p, 150, s_cap(L, p)))
        c["opts"] = TILE_SETS[seed % 5]
    elif shape_of == "wide":
        edge = {0: last_p(L, 32) + 2, 1: last_p(L, 16), 2: last_p(L, 16) + 1, 3: last_p(L, 8)}
        p = edge[seed % 6] if seed % 6 in edge else _ints(rng, last_p(L, 32) + 2, last_p(L, 8))
        s = _ints(rng, 1, min(p, s_cap(L, p)))
        c["opts"] = ("wide",) + TILE_SETS[seed % 5]
    elif shape_of == "far":
        if seed % 8 == 5:
            p, s = 410, 150                                    # a tile fits, the exact pass behind it does not
            assert s > s_cap(L, p) and p <= last_p(L, 32)
        else:
            p = {0: last_p(L, 8) + 1, 2: 8192, 4: 16384}.get(seed % 8) or _ints(rng, last_p(L, 8) + 1, 9000)
            s = _ints(rng, 1, 164)
        band = ((2, 64), (65, 128), (129, 256), (257, 300))[(seed + seed // 4) % 4]      # 1, 2, 4 accumulators per lane; two planes
        c["opts"] = ("wide", "far") + FAR_SETS[(seed // 2) % 4]
    elif shape_of == "far_ragged":
        p = last_p(L, 32) + 1 if seed % 8 == 0 else _ints(rng, last_p(L, 32) + 1, 9000)
        s = _ints(rng, 1, 82)                                  # columns of 0 .. 2 s entries
        c["ragged"] = True
        band = ((2, 64), (65, 128), (129, 256), (257, 300))[(seed + seed // 4) % 4]
        c["opts"] = ("wide", "far", "far_ragged") + FAR_SETS[(seed // 2) % 4]
    elif shape_of == "tile_ragged":
        p = {0: 17, 1: last_p(L, 32)}.get(seed % 8) or _ints(rng, 17, last_p(L, 32))
        s = _ints(rng, 1, max(1, min(82, p // 2)))
        c["ragged"] = True
        band = ((2, 8), (9, 16), (17, 300))[seed % 3]          # tiles of 8, 16, 32 centroids
        c["opts"] = ("tile_ragged",) + PIPE_SETS[(seed // 2) % 2]
    else:                                                      # many
        kind = seed % 3 if route == "many" else 0              # fixed s <= 64 / fixed s > 64 / ragged with the tile-ragged opt-in
        p = _ints(rng, 81 if kind == 1 else 64, 256)           # (a column holds at most p entries)
        s = _ints(rng, 1, 64) if kind == 0 else (_ints(rng, 65, 80) if kind == 1 else _ints(rng, 1, 40))
        c["ragged"] = kind == 2
        band = ((1025, 2048), (2049, 2200))[(seed // 2) % 2]   # 2 and 3 passes of 32 tiles
        c["opts"] = ("many",) + (("tile_ragged",) if kind == 2 else ()) + PIPE_SETS[(seed // 3) % 2]
    if route == "none":
        c["opts"] = tuple(o for o in c["opts"] if o != shape_of)   # (the opt-ins are named as the routes they open)
    lo, hi = K_RANGE[shape_of]
    blo, bhi = band or (lo, hi)
    c["disturb"] = DISTURBANCES[(seed + seed // 3) % 3]
    c["T"] = 1 + seed % 3
    grow = seed % 4 == 1                                       # the second run's K exceeds the first's
    K = _ints(rng, blo + (1 if c["disturb"] == "far+drop" else 0), bhi - (1 if grow and bhi == hi else 0))
    K2 = _ints(rng, K + 1, hi) if grow else _ints(rng, lo, hi)
    K_end = K - (1 if c["disturb"] == "far+drop" else 0)       # the centres the first run ends on
    if seed % 4 == 2:
        K2 = K_end                                             # the one K at which bounds that reset_policy forgot to drop would be believed
    if route == "many" and seed % 8 == 6:
        K2 = _ints(rng, 300, 1024)                             # the second run leaves the route
    small = seed % 4 == 3                                      # a quarter of the seeds
    n = SMALL_N[(2 * ROUTES.index(route) + seed // 4) % len(SMALL_N)] if small else _ints(rng, 200, N_MAX)
    if c["ragged"] and n == 1:
        n = SMALL_N[1]                                         # (one ragged column may be empty: an empty shard has no screen)
    if shape_of == "many" and not small:
        n = 200 + (n - 200) // 2                               # (K up to 2200: the oracle's K n s per call stays in seconds)
    if p > last_p(L, 32) and p * K > 100_000:
        # (the oracle walks a p x K table of tens of MB once per stored entry and centre: n s K per call stays at 12e6 there,
        #  by n where it is drawn, by s where n is one of the small values)
        budget = 12_000_000
        if not small:
            n = max(200, min(n, budget // (s * K)))
        if n * s * K > budget:
            s = max(1, budget // (n * K))
    # the switches of the event forms (SPKM_*, read by the context): the far pipeline's events sorted by key and added up in slabs
    # instead of one by one -- where its accumulation has slabs, csrc/policy.h spkm_accumulate_form -- and, on the lazy
    # 4-lanes-per-point screen, PAIR events (one per mover, out of the cluster left and into the new one), which the policy
    # plans on its own only from 1536 movers up: one by one on seed 1, sorted on seed 5
    c["no_direct"] = "far_events" in c["opts"] and seed % 4 >= 2 and (p <= 5461 or "sliced_sums" in c["opts"])
    c["pair"] = shape_of == "quad" and seed % 4 == 1
    c["switches"] = ((("SPKM_NO_DIRECT_EVENTS",) if c["no_direct"] or (c["pair"] and seed % 8 == 5) else ()) +
                     (("SPKM_FORCE_PAIR_EVENTS",) if c["pair"] else ()))
    c["dup"] = seed % 3 == 0 and K >= 32 and n >= 200
    c.update(p=int(p), s=int(s), K=K, K2=K2, K_end=K_end, n=int(n), lazy="lazy" in c["opts"])
    c["calls"] = 9 if "far_events" in c["opts"] else 8
    return c


def cases(route, mult=1):
    return [(route, seed) for seed in range(SEEDS[route] * mult)]


@functools.lru_cache(maxsize=2)
def _data(route, seed):
    c = draw(route, seed)
    p, n, s, K, K2 = c["p"], c["n"], c["s"], c["K"], c["K2"]
    rng = np.random.default_rng([ROUTES.index(route), seed, 9000])
    empty = tuple(sorted({i for i in (1, n // 2, n - 2) if 0 < i < n})) if c["ragged"] else ()
    X = random_csc(p, n, s, seed=100 * seed + ROUTES.index(route), ragged=c["ragged"], empty_cols=empty).tocsc()
    lab = (np.arange(n) * K) // n
    cen0 = rng.standard_normal((p, K)) * 2.0
    col = np.repeat(np.arange(n), np.diff(X.indptr))
    X.data = np.clip(np.rint((0.3 * X.data + cen0[X.indices, lab[col]]) / UNIT) * UNIT, -CLIP, CLIP)
    gam = s / p
    C0 = gam * cen0 + 0.05 * rng.standard_normal((p, K))
    if c["dup"]:
        C0[:, 1] = C0[:, 0]                                    # a duplicate centre: ties
    # the second run: the planted centres in another order, new ones past them, the same perturbation
    perm = rng.permutation(K)
    base = cen0[:, perm[:K2]] if K2 <= K else np.concatenate([cen0[:, perm], rng.standard_normal((p, K2 - K)) * 2.0], axis=1)
    C2 = gam * base + 0.05 * rng.standard_normal((p, K2))
    for a in (X.data, X.indices, X.indptr, C0, C2):
        a.setflags(write=False)
    return X, gam, C0, C2


def data(case):
    """(X scipy CSC p x n, gamma, C0 p x K, C2 p x K2) -- shared and read-only"""
    return _data(case["route"], case["seed"])


def fixed_stride(X):
    """the stride the library finds (spkm_shard_create_*: every column of nnz / n entries), 0: a ragged shard"""
    n = X.shape[1]
    if n == 0 or X.nnz == 0 or X.nnz % n:
        return 0
    st = X.nnz // n
    return int(st) if np.array_equal(X.indptr, np.arange(n + 1, dtype=np.int64) * st) else 0


# ---- the reference ----
def replay(case, oracle):
    """the calls of the script in order, stepping the oracle (assign -> accumulate -> finalize_centers).  Yields one dict per call:
    run (0 / 1), t (call of its run), K, cin (the centres going in, p x K), want_mind, rebuild (a new engine in front of this call:
    'drop', or the second run), reset (reset_policy in front of it), repeat (the centres of the call before, unchanged), what (the
    disturbance applied to cin, or None), and the expected assign, mind, S, Cnt, nk, cout (the updated centres), dff2."""
    X, gam, C0, C2 = data(case)
    p, n = X.shape
    jc, ir, x = parts(X)
    lazy = case["lazy"]

    def step(cin):
        K = cin.shape[1]
        a, d = oracle.assign(p, n, jc, ir, x, cin, gam)
        S, Cnt, nk = oracle.accumulate(p, n, K, jc, ir, x, a)
        cout = oracle.finalize_centers(S, Cnt, nk, gam, cin)
        return dict(K=K, cin=cin, assign=a, mind=d, S=S, Cnt=Cnt, nk=nk, cout=cout, dff2=float(np.sum((cin - cout) ** 2)))

    kind, _, follow = case["disturb"].partition("+")
    T = case["T"]
    cin, prev, emptied = np.array(C0), None, None
    for t in range(case["calls"]):
        what, rebuild, repeat = None, False, t >= 6
        if repeat:
            cin = prev["cin"]
        elif t > 0:
            cin = prev["cout"].copy()
        if t == T:
            # the largest clusters of the call before, first indices -- by the members that store an entry: an empty column
            # is at distance 0 of every centre and stays with centroid 0 whatever happens to it, so a ragged shard with
            # empty columns never empties that one
            stored = np.diff(X.indptr) > 0
            sizes = np.bincount(prev["assign"][stored], minlength=cin.shape[1])
            if not stored.all():
                sizes[0] = -1
            order = np.argsort(-sizes, kind="stable")
            if kind == "swap":
                a, b = int(order[0]), int(order[1])
                cin[:, [a, b]] = cin[:, [b, a]]
                what = ("swap", a, b)
            else:
                emptied = int(order[0])
                cin[:, emptied] = 40.0 * np.abs(cin).max()
                what = ("far", emptied)
        elif t == T + 1 and kind == "far":
            if follow == "singleton":
                i = int(np.argmax(prev["mind"]))               # [~, iMax] = max(distances): the first index
                cin[:, emptied] = 0.0
                cin[X.indices[X.indptr[i]:X.indptr[i + 1]], emptied] = X.data[X.indptr[i]:X.indptr[i + 1]]
                what = ("singleton", emptied, i)
            else:
                cin = np.ascontiguousarray(np.delete(cin, emptied, axis=1))
                what, rebuild = ("drop", emptied), True
        prev = step(cin)
        yield dict(prev, run=0, t=t, want_mind=(not lazy) or t % 2 == 1, rebuild=rebuild, reset=False, repeat=repeat, what=what)
    cin = np.array(C2)
    for t in range(3):
        if t > 0:
            cin = prev["cout"].copy()
        prev = step(cin)
        # (a second run at the K the first ended on keeps its ENGINE, and with it the assignment buffer the library compares
        #  with its own copy: only reset_policy stands between that run and the first one's bounds)
        yield dict(prev, run=1, t=t, want_mind=(not lazy) or t % 2 == 1, rebuild=t == 0 and case["K2"] != case["K_end"], reset=t == 0,
                   repeat=False, what=None)


# ---- the route, by the library's plan functions ----
@functools.lru_cache(maxsize=None)
def _harnesses():
    import plan_harness as PH
    from test_many_plan import many_lib
    from test_tile_far_plan import tile_far_lib

    return PH, many_lib(), tile_far_lib()


def route_of(case, lds_max, num_cus, K=None):
    """what the first fused call of a run with K centres (None: the case's first run) takes on a device with lds_max bytes of LDS
    and num_cus CUs -- spkm_assign_accumulate_dev's dispatch (csrc/api_lloyd_fused.inc) restated over the plan harnesses, in its
    order: the many-centres screen, the tile-far route, spkm_screen_width, the far screens, the ragged tile screen.  Returns a
    dict: route (the names of ROUTES; 'none': the all-exact kernels), width (centroids per tile or plane), tiles (of that width),
    tile_far, passes (of the many-centres screen, else 0), far_pipe (the stages behind the screen are run_far's), acc_form (the
    kernel of a far-pipeline call's full accumulation: 1 slab / 2 atomics / 3 row slices)."""
    import ctypes as C

    PH, ML, TL = _harnesses()
    X = data(case)[0]
    p, K = case["p"], case["K"] if K is None else K
    fs, nnz, slack, o = fixed_stride(X), int(X.nnz), 48, set(case["opts"])
    has = lambda name: int(name in o)
    a = (p, K, fs, slack, nnz, lds_max, num_cus, 0)
    r = dict(route="none", width=0, tiles=0, tile_far=False, passes=0, far_pipe=False)
    many = ML.many_screen(*a, has("tile_ragged"), has("many"))
    tf = 0 if many else TL.tile_far_screen(*a, has("wide"), has("tile_far"))
    kt = 0 if many or tf else PH.lib().screen_width(*a, has("wide"))
    if many:
        r.update(route="many", width=32, tiles=-(-K // 32), passes=many, far_pipe=True)
    elif tf or kt:
        w = tf or kt
        name = "quad" if PH.lib().screen_quad(w, fs) else ("tile" if w == 32 else "wide")
        r.update(route=name, width=w, tiles=-(-K // w), tile_far=bool(tf), far_pipe=bool(tf))
    else:
        kp = (PH.lib().far_screen(*a, has("wide"), has("far")) if fs > 0 else
              PH.lib().far_screen_ragged(*a, has("far"), has("far_ragged")))
        if kp:
            r.update(route="far" if fs > 0 else "far_ragged", width=kp, tiles=PH.lib().far_planes(K, kp), far_pipe=True)
        else:
            w = PH.lib().tile_screen_ragged(*a, has("tile_ragged"))
            if w:
                r.update(route="tile_ragged", width=w, tiles=-(-K // w), far_pipe=True)
    out = (C.c_int * 4)()
    r["acc_form"] = PH.lib().acc_form(p, lds_max, has("sliced_sums"), 0, out)
    return r


def carries_bounds(case, r):
    """the shard carries distance bounds between the calls of route r: the far pipeline with set_far_bounds, the non-quad tile
    screens of today with set_wide_bounds (the 4-lanes-per-point screen carries its own, by steps: not asserted here)"""
    o = set(case["opts"])
    return ("far_bounds" in o) if r["far_pipe"] else ("wide_bounds" in o and r["route"] in ("tile", "wide"))


def by_events(case, r):
    """... and may move its kept sums by events: the far pipeline with bounds, set_far_events and lazy statistics"""
    return r["far_pipe"] and {"far_bounds", "far_events", "lazy"} <= set(case["opts"])
