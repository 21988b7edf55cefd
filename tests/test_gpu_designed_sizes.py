"""-m gpu: the counting sort, the segment plan and the per-item passes on DESIGNED cluster sizes (tests/designed_sizes.py).

Every accumulation and exact-distance pass runs over one pipeline: k_hist / k_plan_segments / k_plan_segments_wide build a
counting sort by cluster and cut every cluster into work items of at most `seg` points, k_scatter_by_cluster places the
points, and a per-item kernel walks them in batches (k_accumulate_sorted, k_exact_accumulate, k_exact_accumulate_rec and
its variants, k_accumulate_events with and without PAIR, k_events_direct, k_dense_accumulate).  With Gaussian data the
cluster sizes are whatever falls out; here they are dictated: items of 1, 15 / 16 / 17, 255 / 256 / 257 and
2047 / 2048 / 2049 / 4097 points, empty clusters, clusters that become empty and stop being empty, one cluster holding
every point, K = 300 with five clusters populated on both sides of the planner's 256-cluster block, K (K + 1) = 992 and
1056 pair keys around the wide planner's 1024 threads -- in three layouts of the labels (whole waves of one cluster, a
random permutation, runs of 1-99 points), which take the scatter's aggregated path, its per-lane atomics, and both.

Two properties only this fixture can hold the kernels to (tests/test_designed_sizes_cpu.py proves them on the oracle):
  * the arithmetic is exact, so the sums -- after a full pass, after events sorted or applied one by one, added and
    subtracted in any order -- EQUAL the oracle's as numbers: np.array_equal, not a tolerance scaled by the largest sum;
  * the largest distance is exactly 8.0 and is attained by planted points in several clusters, items, waves and -- a
    whole cluster of 2049 of them -- several times per lane, so stats[2], "the first index of the largest distance", is
    the smallest planted index only if every stage breaks the tie by index: per lane, per wave, per item, per cluster
    and in the final reduction.  Continuous data never ties, and passes with any of those tie-breaks removed.
Everything else is held to the bars the suite already has: assignments and distances bit for bit, counts and cluster sizes
exact, obj2 to 1e-12 relative (dist * dist rounds).  Every case proves which kernel form it ran from the library's
read-backs; a form that did not run is a failure, not a pass."""
import numpy as np
import pytest
import torch

import designed_sizes as D
from util import parts, set_switch

pytestmark = pytest.mark.gpu

P = D.P
LAYOUTS = D.LAYOUTS
# the trades of the fused test per size list: L12 as designed (6657 points change cluster); ONE: everything moves into the
# empty cluster 2; SPARSE300: the two long clusters on either side of the planner's block boundary trade places and the
# single member of cluster 255 moves into the empty cluster 1 (clusters 257 and 299 stay as they are)
FUSED_TRADES = {"L12": D.TRADES, "ONE": [(1, 2)], "SPARSE300": [(0, 256), (255, 1)]}
_REF = {}


def ref(oracle, fx, tag, Cm):
    """(assignment, distances, sums, counts, cluster sizes) of the oracle for fixture fx under centres Cm; computed once
    per (fixture, tag), shared and read-only"""
    key = (fx["name"], fx["layout"], fx["ragged"], fx["s"], tag)
    if key not in _REF:
        jc, ir, x = parts(fx["X"])
        a, rd = oracle.assign(P, fx["n"], jc, ir, x, Cm, fx["gamma"])
        S, Cnt, nk = oracle.accumulate(P, fx["n"], fx["K"], jc, ir, x, a)
        for v in (a, rd, S, Cnt, nk):
            v.setflags(write=False)
        _REF[key] = (a, rd, S, Cnt, nk)
    return _REF[key]


def make_shard(ctx, X, bits):
    from sparsifiedkmeans_amd.engine import Shard

    if bits == 16:
        return Shard.from_scipy(ctx, X)
    dev, pad = f"cuda:{ctx.device}", 48
    ir = torch.zeros(X.nnz + pad, dtype=torch.int32, device=dev)
    xv = torch.zeros(X.nnz + pad, dtype=torch.float64, device=dev)
    ir[:X.nnz] = torch.tensor(X.indices.astype(np.int32), device=dev)
    xv[:X.nnz] = torch.tensor(X.data, device=dev)
    return Shard.from_device(ctx, X.shape[0], torch.tensor(X.indptr.astype(np.int64), device=dev), ir, xv, nnz=X.nnz)


def dev_centres(ctx, Cm):
    return torch.tensor(np.ascontiguousarray(Cm.T), device=f"cuda:{ctx.device}")


def unaligned_assign(eng):
    """the engine's assignment buffer moved one int into an allocation of its own: a pointer that is not 16-byte aligned
    selects k_scatter_by_cluster<false> (scalar loads of the assignment)"""
    n = eng.assign.numel()
    eng.assign = torch.zeros(n + 8, dtype=torch.int32, device=eng.assign.device)[1:n + 1]
    assert eng.assign.data_ptr() % 16 == 4 and eng.assign.is_contiguous()


def held(eng, fx, r, tag, mind=True, stats=True, sums=True):
    """the outputs of the call just made against the oracle's (r = ref(...)): assignment (and distances) bit for bit,
    counts and sizes exact, sums EQUAL as numbers, obj2 to 1e-12, the largest distance exactly, and its FIRST index"""
    a, rd, S, Cnt, nk = r
    K, pk = fx["K"], P * fx["K"]
    got = eng.assign.cpu().numpy()
    assert np.array_equal(got, a), (tag, int((got != a).sum()), np.flatnonzero(got != a)[:8])
    if mind:
        assert np.array_equal(eng.mind.cpu().numpy(), rd), tag
    assert np.array_equal(eng.nk.cpu().numpy(), nk), (tag, eng.nk.cpu().numpy()[:16], nk[:16])
    if sums:
        red = eng.reduce.cpu().numpy()
        assert np.array_equal(red[2 * pk:2 * pk + K], nk.astype(np.float64)), tag
        assert np.array_equal(red[pk:2 * pk].reshape(K, P).T, Cnt), tag
        gs = red[:pk].reshape(K, P).T
        bad = np.argwhere(gs != S)
        print(f"[designed] {tag}: sums differ in {len(bad)} of {pk} entries, max |diff| {np.abs(gs - S).max():.3e}")
        assert np.array_equal(gs, S), (tag, len(bad), bad[:4], [(gs[i, k], S[i, k]) for i, k in bad[:4]])
        empty = np.flatnonzero(nk == 0)
        assert np.all(gs[:, empty] == 0.0) and np.all(red[pk:2 * pk].reshape(K, P).T[:, empty] == 0.0), tag
    if stats:
        st = eng.stats.cpu().numpy()
        obj2 = float(np.sum(rd * rd))
        print(f"[designed] {tag}: stats {st.tolist()}, expected max {rd.max()} first at {fx['first']}")
        assert abs(st[0] - obj2) <= 1e-12 * obj2, (tag, st[0], obj2)
        if sums:
            assert abs(eng.reduce[2 * pk + K].item() - obj2) <= 1e-12 * obj2, tag
        assert st[1] == rd.max() and (fx["s"] != 16 or st[1] == 8.0), (tag, st[1])
        assert int(st[2]) == fx["first"] == int(np.argmax(rd)), (tag, int(st[2]), fx["first"], fx["planted"][:6])


# ---- a. spkm_assign_dev + spkm_accumulate_dev ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ragged,bits", [(False, 16), (False, 32), (True, 16), (True, 32)],
                         ids=["stride-ir16", "stride-ir32", "ragged-ir16", "ragged-ir32"])
@pytest.mark.parametrize("name", ["L12", "ONE", "SPARSE300"])
def test_assign_then_accumulate(gpu_ctx, oracle, name, ragged, bits, layout):
    """k_plan_segments over the sizes of the assignment just made, k_scatter_by_cluster<true> and, with the assignment
    one int into its allocation, <false>, then k_accumulate_sorted (the slab form: read back) over fixed-stride and ragged
    columns, 16- and 32-bit row ids"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx = D.fixture(name, layout, ragged=ragged)
    r = ref(oracle, fx, "C", fx["C"])
    assert np.array_equal(r[0], fx["g"]) and np.array_equal(r[4], fx["sizes"])
    eng = LloydEngine(make_shard(gpu_ctx, fx["X"], bits), fx["K"], fx["gamma"])
    assert eng.shard.ir_bits == bits
    c = dev_centres(gpu_ctx, fx["C"])
    for form in ("aligned", "one int in"):
        if form != "aligned":
            unaligned_assign(eng)
        eng.assign_step(c)
        eng.accumulate_step()
        torch.cuda.synchronize()
        assert eng.last_assign_tile()[4] == 1, eng.last_assign_tile()
        held(eng, fx, r, f"assign+accumulate {name} {layout} ragged={ragged} ir{bits} {form}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_assign_then_accumulate_long_columns(gpu_ctx, oracle, layout):
    """s = 70: the "columns longer than one wave" loop of k_accumulate_sorted.  gamma = 35 / 128; the planted points
    still share one distance, whatever f64 makes of sqrt(280)"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx = D.fixture("L12", layout, s=70)
    r = ref(oracle, fx, "C", fx["C"])
    assert np.array_equal(r[0], fx["g"]) and np.array_equal(np.flatnonzero(r[1] == r[1].max()), fx["planted"])
    eng = LloydEngine(make_shard(gpu_ctx, fx["X"], 16), fx["K"], fx["gamma"])
    c = dev_centres(gpu_ctx, fx["C"])
    eng.assign_step(c)
    eng.accumulate_step()
    torch.cuda.synchronize()
    assert eng.last_assign_tile()[4] == 1
    held(eng, fx, r, f"assign+accumulate s=70 {layout}")


# ---- b. the fused call ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("want_mind", [True, False], ids=["mind", "no-mind"])
@pytest.mark.parametrize("rec", [True, False], ids=["records", "no-rec"])
@pytest.mark.parametrize("name", ["L12", "ONE", "SPARSE300"])
def test_fused_call_three_times(gpu_ctx, oracle, monkeypatch, name, rec, want_mind, layout):
    """spkm_assign_accumulate_dev with C, with C again, with traded centres: the full pass's sort and plan, then
    k_exact_accumulate_rec (record layout) or k_exact_accumulate (SPKM_NO_REC).  Without d_mind the record form streams
    only the clusters whose centroid or membership changed -- nothing in the second call, exactly the members of the
    traded clusters in the third (6657 on L12) -- and takes the others' sums and statistics from its cache: the planted
    points sit in cached and in streamed clusters, and stats[2] must be the smallest of them in every call."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx = D.fixture(name, layout)
    cycles = FUSED_TRADES[name]
    T = D.trade(fx["C"], cycles)
    refs = {"C": ref(oracle, fx, "C", fx["C"]), "T": ref(oracle, fx, "fused trade", T)}
    assert np.array_equal(refs["T"][0], D.traded_labels(fx["g"], cycles))
    touched = sorted({k for c in cycles for k in c})
    streamed = int(refs["T"][4][touched].sum())
    assert name != "L12" or streamed == 6657
    if not rec:
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_REC")
    eng = LloydEngine(make_shard(gpu_ctx, fx["X"], 16), fx["K"], fx["gamma"])
    for call, (tag, Cm) in enumerate((("C", fx["C"]), ("C", fx["C"]), ("T", T))):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm), want_mind=want_mind)
        torch.cuda.synchronize()
        what = f"fused {name} {layout} rec={rec} mind={want_mind} call {call} ({tag})"
        assert eng.last_path_info()[0] == 1, what                               # the screen path: run_screen's passes
        pts, streamed_now = eng.last_assign_tile()[3], eng.exact_pass_points()[1]
        print(f"[designed] {what}: staged per wave {pts}, streamed {streamed_now}")
        assert (pts == 16) == rec, (what, pts)                                    # 16: the pipelined record kernel
        if rec:
            want = fx["n"] if (want_mind or call == 0) else (0 if call == 1 else streamed)
            assert streamed_now == want, (what, streamed_now, want)
        held(eng, fx, refs[tag], what, mind=want_mind)


# ---- c. distances on demand ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["L12", "SPARSE300"])
def test_streaming_distances_with_the_kept_sort_and_with_a_fresh_one(gpu_ctx, oracle, name, layout):
    """spkm_distances_stats_dev's streaming form (k_exact_accumulate_rec<ACCUM = false> + k_reduce_stats_n over the items):
    right after a fused call, on the counting sort that call left behind; then for ANOTHER assignment in another buffer
    (the traded centres' -- the kept sort no longer describes it: k_hist, plan and scatter run afresh), aligned and one
    int into its allocation; then after reset_policy()"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx = D.fixture(name, layout)
    cycles = FUSED_TRADES[name]
    T = D.trade(fx["C"], cycles)
    rC, rT = ref(oracle, fx, "C", fx["C"]), ref(oracle, fx, "fused trade", T)
    sh = make_shard(gpu_ctx, fx["X"], 16)
    eng = LloydEngine(sh, fx["K"], fx["gamma"])
    c, t = dev_centres(gpu_ctx, fx["C"]), dev_centres(gpu_ctx, T)
    eng.assign_accumulate_step(c, want_mind=False)
    eng.mind.fill_(-1.0)
    eng.stats.fill_(-1.0)
    eng.distances(c)
    torch.cuda.synchronize()
    assert eng.last_assign_tile()[5] == 1, eng.last_assign_tile()
    held(eng, fx, rC, f"distances kept sort {name} {layout}", sums=False)
    for form in ("aligned", "one int in"):
        if form == "aligned":
            eng.assign = torch.tensor(rT[0], device=eng.assign.device)
        else:
            unaligned_assign(eng)
            eng.assign.copy_(torch.tensor(rT[0], device=eng.assign.device))
        eng.mind.fill_(-1.0)
        eng.stats.fill_(-1.0)
        eng.distances(t)
        torch.cuda.synchronize()
        assert eng.last_assign_tile()[5] == 1, eng.last_assign_tile()
        a, rd = rT[0], rT[1]
        assert np.array_equal(eng.mind.cpu().numpy(), rd), (name, layout, form)
        st = eng.stats.cpu().numpy()
        print(f"[designed] distances fresh sort {name} {layout} {form}: stats {st.tolist()} first {fx['first']}")
        assert abs(st[0] - np.sum(rd * rd)) <= 1e-12 * np.sum(rd * rd) and st[1] == 8.0 and int(st[2]) == fx["first"], (form, st)
    sh.reset_policy()
    eng.assign = torch.tensor(rC[0], device=eng.assign.device)
    eng.mind.fill_(-1.0)
    eng.stats.fill_(-1.0)
    eng.distances(c)
    torch.cuda.synchronize()
    assert eng.last_assign_tile()[5] == 1
    assert np.array_equal(eng.mind.cpu().numpy(), rC[1])
    st = eng.stats.cpu().numpy()
    assert st[1] == 8.0 and int(st[2]) == fx["first"], st


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("how", ["ragged", "no-rec"])
@pytest.mark.parametrize("name", ["L12", "SPARSE300"])
def test_generic_distances_and_their_statistics(gpu_ctx, oracle, monkeypatch, name, how, layout):
    """the generic form (k_point_distances + k_mind_stats + k_reduce_stats; read back) on a ragged shard and, SPKM_NO_REC,
    on a fixed-stride shard without the record layout: the caller's assignment, statistics from the distances written"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx = D.fixture(name, layout, ragged=how == "ragged")
    r = ref(oracle, fx, "C", fx["C"])
    if how == "no-rec":
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_REC")
    eng = LloydEngine(make_shard(gpu_ctx, fx["X"], 16 if how == "no-rec" else 32), fx["K"], fx["gamma"])
    c = dev_centres(gpu_ctx, fx["C"])
    eng.assign_accumulate_step(c, want_mind=False)
    eng.mind.fill_(-1.0)
    eng.stats.fill_(-1.0)
    eng.distances(c)
    torch.cuda.synchronize()
    assert eng.last_assign_tile()[5] == 2, eng.last_assign_tile()
    held(eng, fx, r, f"generic distances {name} {layout} {how}")


@pytest.mark.parametrize("bits", [16, 32])
def test_one_centroid_stream(gpu_ctx, oracle, bits):
    """K = 1 (the k-means++ rounds): k_exact_dist1 streams the shard; planted points at indices 1500, 1501 and 2499 lie
    in different waves and workgroups, and the first of them is the answer"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx = D.fixture("K1", "sorted")
    assert fx["planted"].tolist() == list(D.K1_TIES) and fx["first"] == 1500
    r = ref(oracle, fx, "C", fx["C"])
    eng = LloydEngine(make_shard(gpu_ctx, fx["X"], bits), 1, fx["gamma"])
    eng.assign_step(dev_centres(gpu_ctx, fx["C"]))
    eng.accumulate_step()
    torch.cuda.synchronize()
    t = eng.last_assign_tile()
    assert t[0] == 0 and t[1] == 1 and t[3] >= 16 and t[4] == 1, t                # the K = 1 stream, then the slab form
    held(eng, fx, r, f"K = 1 ir{bits}")


# ---- d. lazy incremental sums on designed movers ----
EVENT_SWITCHES = [((), ("L12",)), (("SPKM_NO_DIRECT_EVENTS",), ("L12",)),
                  (("SPKM_NO_DIRECT_EVENTS", "SPKM_FORCE_PAIR_EVENTS"), ("L12", "L32", "L31")),
                  (("SPKM_NO_DIRECT_EVENTS", "SPKM_NO_PAIR_EVENTS"), ("L12",))]
EVENT_CASES = [(sw, name) for sw, names in EVENT_SWITCHES for name in names]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("switches,name", EVENT_CASES, ids=[("+".join(s) or "default") + "-" + nm for s, nm in EVENT_CASES])
def test_lazy_sums_follow_designed_movers(gpu_ctx, oracle, monkeypatch, switches, name, layout):
    """set_lazy_stats(True), no distances: C, C, the small trade, the whole trade, C.  The first call is the sums-only full
    pass; the second knows no mover count and lets the device choose (no movers: the events); the two trade calls see
    a previous count of 0 and of 513 movers and are INCREMENTAL -- events applied one by one by default, sorted into
    items of at most 256 with SPKM_NO_DIRECT_EVENTS (runs of 1 / 255 / 257, then of 2047 / 2048 / 2049 per key), pair
    events with SPKM_FORCE_PAIR_EVENTS (K (K + 1) = 156, 992 and 1056 keys) -- which is asserted: a full pass there
    would make this test pass vacuously.  (The trade is made in two steps because the policy follows by events only a
    call whose predecessor moved at most a third of the points, policy.h few_movers: after the 6144 movers of the large
    trade the last call is a full pass again, which is asserted too.)  Cluster 1 is emptied into the empty cluster 0 and
    filled again: its sums and counts must be exactly 0 in between.  After every call the sums EQUAL the oracle's."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    fx = D.fixture(name, layout)
    K = fx["K"]
    last = [(K - 2, K - 1)] if name == "L32" else []
    T1, T2 = D.trade(fx["C"], D.TRADE_SMALL + last), D.trade(fx["C"], D.TRADES + last)
    refs = {"C": ref(oracle, fx, "C", fx["C"]), "T1": ref(oracle, fx, "small trade", T1), "T2": ref(oracle, fx, "whole trade", T2)}
    assert np.array_equal(refs["T2"][0], D.traded_labels(fx["g"], D.TRADES + last))
    for sw in switches:
        set_switch(monkeypatch, gpu_ctx, sw)
    direct = "SPKM_NO_DIRECT_EVENTS" not in switches
    pair = "SPKM_FORCE_PAIR_EVENTS" in switches
    sh = make_shard(gpu_ctx, fx["X"], 16)
    sh.set_lazy_stats(True)
    eng = LloydEngine(sh, K, fx["gamma"])
    prev = None
    for call, tag in enumerate(("C", "C", "T1", "T2", "C")):
        Cm = {"C": fx["C"], "T1": T1, "T2": T2}[tag]
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm), want_mind=False)
        torch.cuda.synchronize()
        md, ev = eng.last_screen_mode(), eng.last_events_form()
        movers = -1 if prev is None else int(np.count_nonzero(refs[tag][0] != prev))
        prev = refs[tag][0]
        what = f"lazy {name} {layout} {'+'.join(switches) or 'default'} call {call} ({tag}): sums {md[6]} events {ev} movers {movers}"
        print("[designed]", what)
        assert eng.last_path_info()[0] == 1, what
        held(eng, fx, refs[tag], what, mind=False, stats=False)
        if call == 0:
            assert md[6] == 3 and ev[0] == 0, what                              # the sums-only full pass
        elif call == 1:
            # both forms queued and the device opened the events -- unless the shard, its points in arbitrary order, was
            # regrouped by cluster in front of this call (policy.h, regroup_wanted), which costs it the kept sort: a full pass
            assert movers == 0 and (md[6], ev[0]) in (((2, 1),) if layout == "sorted" else ((2, 1), (3, 0))), what
        elif call in (2, 3):
            assert movers == (513 if call == 2 else 6144) + (80 if last and call == 2 else 0), what
            assert md[6] == (4 if direct else 2) and ev == ((2 if direct else 1), int(pair)), what
            if call == 2:                                                         # cluster 1's single member went to cluster 0
                red, pk = eng.reduce.cpu().numpy(), P * K
                assert refs[tag][4][0] == 1 and refs[tag][4][1] == 0
                assert not red[:2 * pk].reshape(2, K, P)[:, 1].any() and red[2 * pk + 1] == 0.0, what
        else:
            assert movers == 6657 + (80 if last else 0) and md[6] == 3 and ev[0] == 0, what   # too many moved before: a full pass
            red, pk = eng.reduce.cpu().numpy(), P * K
            assert not red[:2 * pk].reshape(2, K, P)[:, 0].any() and red[2 * pk] == 0.0, what  # ... and cluster 0 is empty again
    eng.distances(dev_centres(gpu_ctx, fx["C"]))
    torch.cuda.synchronize()
    held(eng, fx, refs["C"], f"lazy {name} {layout} distances at the end", sums=False)
    sh.set_lazy_stats(False)


# ---- e. the dense accumulation ----
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["D9", "SPARSE300"])
def test_dense_accumulate(gpu_ctx, name, layout):
    """spkm_dense_accumulate_dev (k_hist, k_plan_segments with segments of 256, k_scatter_by_cluster, k_dense_accumulate)
    takes the caller's assignment: the designed labels, dense rows of p = 100 with the same dyadic values -- in one call,
    in two chunks split at an odd index, and with the assignment one int into its allocation"""
    from sparsifiedkmeans_amd.engine import dense_accumulate_device

    sizes = D.SIZE_LISTS[name]
    K, p = len(sizes), 100
    g = D.labels(sizes, layout, D.SEED[name])
    Xd = D.dense_rows(g, p, D.SEED[name])
    n = g.size
    want = np.zeros((K, p))
    np.add.at(want, g, Xd)
    dev = f"cuda:{gpu_ctx.device}"
    xd, gd = torch.tensor(Xd, device=dev), torch.tensor(g, device=dev)
    off = torch.zeros(n + 8, dtype=torch.int32, device=dev)[1:n + 1]
    off.copy_(gd)
    assert off.data_ptr() % 16 == 4
    for form, chunks, lab in (("one call", [(0, n)], gd), ("two chunks", [(0, 1001), (1001, n)], gd), ("one int in", [(0, n)], off)):
        sums = torch.zeros((K, p), dtype=torch.float64, device=dev)
        cnt = torch.zeros(K, dtype=torch.float64, device=dev)
        for lo, hi in chunks:
            dense_accumulate_device(gpu_ctx, xd[lo:hi], lab[lo:hi], sums, cnt)
        torch.cuda.synchronize()
        assert np.array_equal(cnt.cpu().numpy(), np.asarray(sizes, np.float64)), (name, layout, form)
        got = sums.cpu().numpy()
        assert np.array_equal(got, want), (name, layout, form, np.abs(got - want).max())
