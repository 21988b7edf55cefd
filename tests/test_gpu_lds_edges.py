"""-m gpu: the Lloyd kernels on both sides of every LDS-size threshold in p.

Which kernel a Lloyd call runs is decided by comparisons of a formula in p (rows) and s (entries per column) with the
LDS size of the device (api_lloyd.hip, api_lloyd_fused.inc, policy.h).  A formula one row or 16 bytes short does not
fault on this hardware -- LDS reads out of range return zero, writes are dropped -- it gives a wrong distance or a lost
sum for the last row or the last staged point; a formula too generous makes one value of p fail to launch.  Every case
here sits on the last p that fits or on the first that does not, proves which kernel form it ran (spkm_last_path_info,
spkm_last_screen_mode, spkm_last_assign_tile) and holds every output to the oracle: assignments and distances bit for
bit, counts and cluster sizes exactly, sums to 1e-12 (full passes) / 1e-10 (incremental calls) of the largest sum, centres
to 1e-9.  Rows p-2 and p-1 carry large values in a share of the columns and in one centroid, which those columns must win.

The limits are computed HERE, in plain integers, from the LDS size the device reports (Context.device_info), restated
from the host code and not taken from it.  With 160 KB (163840 B, what gfx950 is expected to report) they fall at
p = 318 | 319, 638 | 639, 1278 | 1279 (exact tiles of 64 / 32 / 16 centroids; 1278 | 1279 also the screen), 1136 | 1137 (a
last tile of <= 4 centroids carried by the tile before), 409 | 410 (s = 150: eight staged points per wave), 3712 | 3713
(K = 1 stream, s = 64), 1484 | 1485 (streaming distances, s = 64) and 5461 | 5462 (64-KB accumulation slab)."""
import numpy as np
import pytest
import torch

from util import parts, random_csc, set_switch

pytestmark = pytest.mark.gpu

SIDES = ("fits", "over")


# ---- the limits, restated (bytes of LDS; L = the device's LDS per workgroup) ----
def fits_tile(L, p, kt):            # k_assign_tile<kt>: (p + 1) rows of kt doubles + the work-ticket counter
    return (p + 1) * kt * 8 + 16 <= L


def fits_screen(L, p):              # the screen's f32 tile of 32 centroids, row p all zero
    return (p + 1) * 32 * 4 + 16 <= L


def fits_phase2(L, p, s):           # the exact pass behind the screen: centroid + slab + 8 staged points in each of 16 waves
    return p * 20 + 1024 + 16 * 8 * (s | 1) * 8 <= L


def fits_carry(L, p):               # ... and 16 B per row more: a last tile of <= 4 centroids rides on the tile before
    return (p + 1) * (32 * 4 + 16) + 16 <= L


def fits_pipe(L, p, s):             # the pipelined record kernel / the streaming distances: 16 waves x 16 points
    return p * 20 + 16 + 256 * (s | 1) * 8 + 1024 <= L


def exact_pts(L, p, s):             # points staged per wave by k_exact_accumulate
    return max(8, min(64, (L - p * 20 - 16 - 1024) // 16 // ((s | 1) * 8)) & ~7)


def fits_k1(L, p, s):               # k_exact_dist1: the centroid + 16 staged points in each of 16 waves
    return p * 8 + 1024 + 256 * (s | 1) * 8 <= L


def k1_pts(L, p, s):
    return max(16, min(64, (L - p * 8 - 1024) // 16 // ((s | 1) * 8)) & ~15)


def fits_slab(L, p):                # k_accumulate_sorted's slab: a double and a counter per row, at most 64 KB
    return p * 12 <= min(L, 64 * 1024)


def pick_kt(L, p, K):
    """the tile width of the exact assignment: of the widths that fit, the one with the fewest padded slots; the wider on ties"""
    best = (None, 0)
    for kt in (16, 32, 64):
        if fits_tile(L, p, kt):
            slots = -(-K // kt) * kt
            if best[0] is None or slots < best[0] or (slots == best[0] and kt > best[1]):
                best = (slots, kt)
    return best[1]


def largest(fits):
    """largest p >= 0 with fits(p); fits holds up to a limit and not beyond it"""
    lo, hi = 0, 1 << 22
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid - 1)
    return lo


def edge(fits, side):
    p = largest(fits) + (side == "over")
    assert p >= 8 and fits(p) == (side == "fits")
    return p


def lds_of(ctx):
    return int(ctx.device_info()["lds_bytes"])


# ---- inputs ----
def spiked(X, every=11):
    """X with large values in rows p-2 and p-1 of every `every`-th column that has two entries (they replace its last two
    entries: rows stay ascending, a fixed stride stays fixed).  Returns (X, the value, the columns)."""
    X = X.tocsc().copy()
    p, n = X.shape
    big = 8.0 * float(np.abs(X.data).max())
    cols = []
    for j in range(3, n, every):
        b = X.indptr[j + 1]
        if b - X.indptr[j] >= 2:
            X.indices[b - 2:b] = (p - 2, p - 1)
            X.data[b - 2:b] = big
            cols.append(j)
    return X, big, np.array(cols)


def spiked_centres(rng, p, K, gam, big, scale=1.0):
    """p x K centres ~ gam * N(0, scale^2) (so that centres / gam compare with the data); the last one holds the spike"""
    Cm = gam * scale * rng.standard_normal((p, K))
    Cm[p - 2:, K - 1] = gam * big
    return Cm


def make_shard(ctx, X, bits=16):
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


def held(eng, oracle, X, Cm, gam, mind=True, tol=1e-12, stats=None, centres=False, tag=""):
    """the outputs of the call just made against the oracle; returns (assignment, distances) of the oracle"""
    p, n = X.shape
    K = Cm.shape[1]
    jc, ir, x = parts(X)
    ra, rd = oracle.assign(p, n, jc, ir, x, Cm, gam)
    assert np.array_equal(eng.assign.cpu().numpy(), ra), tag
    if mind:
        assert np.array_equal(eng.mind.cpu().numpy(), rd), tag
    S, Cnt, nk = oracle.accumulate(p, n, K, jc, ir, x, ra)
    red = eng.reduce.cpu().numpy()
    pk = p * K
    assert np.array_equal(red[pk:2 * pk].reshape(K, p).T, Cnt), tag
    assert np.array_equal(red[2 * pk:2 * pk + K], nk.astype(float)), tag
    assert np.array_equal(eng.nk.cpu().numpy(), nk), tag
    err, top = np.abs(red[:pk].reshape(K, p).T - S).max(), max(np.abs(S).max(), 1e-300)
    print(f"[lds-edges] {tag} sums err / max|S| = {err / top:.3e}")
    assert err <= tol * top, tag
    if (mind if stats is None else stats):
        st = eng.stats.cpu().numpy()
        assert abs(st[0] - np.sum(rd * rd)) <= 1e-12 * np.sum(rd * rd), tag
        assert st[1] == rd.max() and int(st[2]) == int(np.argmax(rd)), tag
    if centres:
        c = dev_centres(eng.ctx, Cm)
        eng.allreduce_step()
        eng.finalize_step(c)
        want = oracle.finalize_centers(S, Cnt, nk, gam, Cm)
        assert np.abs(c.cpu().numpy().T - want).max() <= 1e-9 * np.abs(want).max(), tag
    return ra, rd


# ---- a. exact tiled assignment: the tile width ----
@pytest.mark.parametrize("K", [64, 17, 65])
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("kt", [64, 32, 16])
def test_exact_tiles_on_both_sides_of_each_tile_width(gpu_ctx, oracle, monkeypatch, kt, side, K):
    """SPKM_NO_SCREEN=1: the fused call runs k_assign_tile at the width pick_kt takes -- K = 64 pads to the same slot count
    at every width, so the widest that fits wins; K = 17 and 65 prefer narrower tiles -- or, past the 16-centroid tile,
    k_assign_generic; then the accumulation.  The width is read back."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    p = edge(lambda q: fits_tile(L, q, kt), side)
    s, n = 20, 2003
    gam = s / p
    X, big, cols = spiked(random_csc(p, n, s, seed=p + K))
    Cm = spiked_centres(np.random.default_rng(K + kt), p, K, gam, big)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN")
    eng = LloydEngine(make_shard(gpu_ctx, X), K, gam)
    eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
    torch.cuda.synchronize()
    assert eng.last_path_info()[0] == 0
    want = pick_kt(L, p, K)
    if K == 64:
        assert want == max([w for w in (16, 32, 64) if fits_tile(L, p, w)], default=0)
    t = eng.last_assign_tile()
    assert t[0] == want and t[1] == (-(-K // want) if want else 1), (t, want, p)
    assert t[4] == 1 and t[3] == 0, t
    ra, _ = held(eng, oracle, X, Cm, gam, centres=True, tag=f"tiles p={p} K={K}")
    assert np.all(ra[cols] == K - 1)


@pytest.mark.parametrize("bits,ragged,K", [(32, False, 64), (16, True, 65), (32, True, 17), (32, False, 65)])
@pytest.mark.parametrize("side", SIDES)
def test_last_tile_width_and_generic_kernel_with_ragged_columns_and_wide_row_ids(gpu_ctx, oracle, monkeypatch, side, bits, ragged, K):
    """the limit between the 16-centroid tile and k_assign_generic again: 32-bit row ids, ragged columns (lanes past a
    column's end read the all-zero row p, the row BEHIND the spiked ones) and an empty column"""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    p = edge(lambda q: fits_tile(L, q, 16), side)
    s, n = 18, 1501
    gam = s / p
    X, big, cols = spiked(random_csc(p, n, s, seed=7 * K + bits, ragged=ragged, empty_cols=(0, 14) if ragged else ()))
    Cm = spiked_centres(np.random.default_rng(K + bits), p, K, gam, big)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_SCREEN")
    eng = LloydEngine(make_shard(gpu_ctx, X, bits), K, gam)
    assert eng.shard.ir_bits == bits
    eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
    torch.cuda.synchronize()
    t = eng.last_assign_tile()
    assert eng.last_path_info()[0] == 0 and t[0] == pick_kt(L, p, K) and (t[0] == 0) == (side == "over"), t
    ra, _ = held(eng, oracle, X, Cm, gam, tag=f"generic p={p} K={K} bits={bits} ragged={ragged}")
    assert cols.size > 50 and np.all(ra[cols] == K - 1)


# ---- b. screen eligibility ----
def _mixture(p, n, K, s, seed, noise):
    """fixed-stride shard of a planted mixture (no sketch: the rows themselves are sampled), spiked; centres / gam at the
    planted means, the last one holding the spike"""
    from sparsifiedkmeans_amd import synth

    X, centres, labels = synth.gmm_dense(p, n, K, seed=seed, noise=noise)
    Y = synth.sparsify_dense(X, s, np.random.default_rng(seed + 1))
    assert Y.nnz == n * s
    Y, big, cols = spiked(Y)
    gam = s / p
    base = gam * centres
    base[p - 2:, K - 1] = gam * big
    return Y, gam, base, cols


def _drift_sequence(base, K, calls):
    """teacher-forced centres: first call, small drifts, a call that moves nothing (the same centres again), a jump that
    moves about a third of the points (a third of the centroids trade places), drifts again"""
    sc = np.abs(base[:-2]).max()
    jump = base.copy()
    q = max(2, K // 3)
    jump[:-2, :q] = base[:-2, np.roll(np.arange(q), 1)]       # (rows p-2, p-1 stay: the spike keeps its centroid)
    seq = [("drift", 0.0), ("drift", 6e-3), ("drift", 9e-3), ("drift", 9e-3), ("drift", 12e-3), ("jump", 12e-3), ("jump", 15e-3),
           ("drift", 15e-3), ("drift", 18e-3), ("drift", 18e-3)][:calls]
    for what, eps in seq:
        noise = np.random.default_rng(200 + int(eps * 1e4)).standard_normal(base.shape)
        noise[-2:] = 0.0                                     # (the spiked rows stay put: the spiked columns keep their centroid)
        yield what, (jump if what == "jump" else base) + eps * sc * noise


@pytest.mark.parametrize("K", [2, 40, 100, 130])
@pytest.mark.parametrize("s", [4, 26, 64])
@pytest.mark.parametrize("side", SIDES)
def test_screen_on_both_sides_of_its_tile_limit(gpu_ctx, oracle, monkeypatch, side, s, K):
    """The last p whose f32 tile (p + 1 rows, the last one all zero, directly behind the spiked rows) fits, and the next:
    an eager run of 6 calls and a lazy run of 10 through drifts, a call without movers and a jump.  Below the limit every
    call is a screen call and the lazy run moves its sums by sorted events (2), one by one (4) and by full sums-only
    passes (3); above it every call runs the all-exact kernels, lazy shard or not, and distances come on request."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    p = edge(lambda q: fits_screen(L, q), side)
    assert fits_phase2(L, p, s) and fits_pipe(L, largest(lambda q: fits_screen(L, q)), s)
    n = 5003
    Y, gam, base, cols = _mixture(p, n, K, s, seed=100 * s + K, noise=0.7)
    shard = make_shard(gpu_ctx, Y)
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_PRUNE")
    want_path = 1 if side == "fits" else 0
    # eager: every call with distances and statistics, full passes
    eng = LloydEngine(shard, K, gam)
    for it, (what, Cm) in enumerate(_drift_sequence(base, K, 6)):
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        torch.cuda.synchronize()
        assert eng.last_path_info()[0] == want_path, (it, what)
        ra, _ = held(eng, oracle, Y, Cm, gam, centres=True, tag=f"eager p={p} s={s} K={K} call {it}")
        assert np.all(ra[cols] == K - 1)
    # lazy: no distances; events where the screen runs
    shard.reset_policy()
    shard.set_lazy_stats(True)
    eng = LloydEngine(shard, K, gam)
    forms = []
    for it, (what, Cm) in enumerate(_drift_sequence(base, K, 10)):
        c = dev_centres(gpu_ctx, Cm)
        eng.assign_accumulate_step(c, want_mind=False)
        torch.cuda.synchronize()
        assert eng.last_path_info()[0] == want_path, (it, what, forms)
        forms.append(eng.last_screen_mode()[6])
        ra, rd = held(eng, oracle, Y, Cm, gam, mind=False, tol=1e-10, tag=f"lazy p={p} s={s} K={K} call {it} form {forms[-1]}")
        assert np.all(ra[cols] == K - 1)
        if it in (4, 9):                                     # the distances and their statistics, on request
            eng.distances(c)
            assert np.array_equal(eng.mind.cpu().numpy(), rd)
            st = eng.stats.cpu().numpy()
            assert abs(st[0] - np.sum(rd * rd)) <= 1e-12 * np.sum(rd * rd) and st[1] == rd.max() and int(st[2]) == int(np.argmax(rd))
    shard.set_lazy_stats(False)
    if side == "fits":
        assert forms[0] == 3 and {2, 3, 4} <= set(forms), forms
    else:
        assert set(forms) == {0}, forms


# ---- c. a last tile of <= 4 centroids carried by the tile before ----
@pytest.mark.parametrize("K", [66, 100])
@pytest.mark.parametrize("where", ["carry-fits", "carry-over", "screen-fits"])
def test_carried_last_tile_on_both_sides_of_its_limit(gpu_ctx, oracle, monkeypatch, where, K):
    """K = 66 / 100: a last tile of 2 / 4 centroids.  Below the limit it rides on the tile before as a fifth centroid per
    lane (16 B per row more LDS: pl_last 5), above it gets a narrow tile of its own (pl_last 1) -- up to the last p the
    screen takes.  More than a tenth of the points are won by last-tile centroids (the spiked columns by K - 2), and K - 1
    has a twin in tile 0: the tie goes to the lower index.  Eight calls as the policy moves (plain, then the two-phase form on these separated clusters),
    then the hinted form (test aid SPKM_FORCE_FORM=3); SPKM_NO_BOUNDS=1 keeps every point on the screen in every call."""
    from sparsifiedkmeans_amd import synth
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    p = edge(lambda q: fits_carry(L, q), "over" if where == "carry-over" else "fits") if where != "screen-fits" else edge(lambda q: fits_screen(L, q), "fits")
    assert fits_screen(L, p)
    want_pl = 5 if fits_carry(L, p) else 1
    s, n = 51, 6007
    assert fits_phase2(L, p, s)
    gam = s / p
    rng = np.random.default_rng(K + p)
    cen = rng.standard_normal((p, K))
    twin = K - 1                                             # a last-tile centroid ...
    cen[:, 3] = cen[:, twin]                                 # ... and its twin in tile 0
    last0 = (K - 1) // 32 * 32                               # first centroid of the last tile
    labels = rng.integers(0, last0, n)
    labels[labels == 3] = 4                                  # (nobody is planted on the twins but the five points below)
    if K - 2 > last0:                                        # (K - 2 holds the spike and K - 1 is the twin: nobody is planted on them)
        share = rng.random(n) < 0.15
        labels[share] = rng.integers(last0, K - 2, int(share.sum()))
    mine = np.array([0, 1, 2, 4, 5])                          # (column 3 is a spiked one)
    labels[mine] = twin
    X = cen[:, labels] + 0.2 * rng.standard_normal((p, n))
    Y = synth.sparsify_dense(X, s, rng)
    assert Y.nnz == n * s
    Y, big, cols = spiked(Y, every=9)                        # a ninth of the columns: their winner is K - 2, in the last tile
    cols = cols[labels[cols] != twin]
    spike_k = K - 2                                          # (the spike: the other end of the last tile, K - 2)
    Cm = cen.copy()                                          # (the members' means: gam * S / Cnt of values X / gam)
    Cm[p - 2:, spike_k] = gam * big
    set_switch(monkeypatch, gpu_ctx, "SPKM_NO_BOUNDS")
    eng = LloydEngine(make_shard(gpu_ctx, Y), K, gam)
    c = dev_centres(gpu_ctx, Cm)
    modes = []

    def call(tag):
        eng.assign_accumulate_step(c)
        torch.cuda.synchronize()
        md = eng.last_screen_mode()
        modes.append(md[0])
        print(f"[lds-edges] carried {where} p={p} K={K} {tag}: form {md[0]}, listed {md[1]}, ambiguous {md[2]}, early {md[3]}")
        assert eng.last_path_info()[0] == 1, (tag, modes)
        assert eng.last_assign_tile()[2] == want_pl, (tag, eng.last_assign_tile(), p)
        ra, _ = held(eng, oracle, Y, Cm, gam, tag=f"carried {where} p={p} K={K} {tag} mode {modes[-1]}")
        assert not np.any(ra == twin) and np.all(ra[mine] == 3)       # the tie: the lower index
        assert np.count_nonzero(ra >= last0) > 0.1 * n and np.all(ra[cols] == spike_k)

    for it in range(8):
        call(f"call {it}")
    assert modes[0] == 0 and 1 in modes, modes                       # plain and two-phase, by the policy
    monkeypatch.setenv("SPKM_FORCE_FORM", "3")
    gpu_ctx.reload_switches()
    for it in range(2):
        call(f"hinted {it}")
    assert modes[-1] == 2 and eng.last_screen_rounds()[0] < eng.last_screen_rounds()[1], modes


# ---- d. points staged per wave ----
def _stage_case(L, name):
    """(p, s, no_rec, expected path, expected points per wave) of a fused exact-pass case"""
    if name.startswith("tier"):                              # no record layout: k_exact_accumulate at every tier
        t, p = int(name[4:]), 300
        s = next(s for s in range(64, 0, -1) if fits_phase2(L, p, s) and exact_pts(L, p, s) == t)
        return p, s, True, 1, t
    if name.startswith("long16"):                            # columns of 75 entries: the 16-lanes-per-point screen, no pipeline
        s = 75
        p = edge(lambda q: (L - q * 20 - 16 - 1024) // 16 // ((s | 1) * 8) >= 16, name[7:])
        return p, s, False, 1, exact_pts(L, p, s)
    s = 150                                                  # "long8-*": the second eligibility limit, eight points per wave
    p = edge(lambda q: fits_phase2(L, q, s), name[6:])
    return p, s, False, 1 if fits_phase2(L, p, s) else 0, 8 if fits_phase2(L, p, s) else 0


@pytest.mark.parametrize("name", ["tier64", "tier56", "tier48", "tier40", "tier32", "tier24", "tier16", "long16-fits", "long16-over",
                                  "long8-fits", "long8-over"])
def test_fused_exact_pass_stages_every_number_of_points_per_wave(gpu_ctx, oracle, monkeypatch, name):
    """k_exact_accumulate stages pts = min(64, room / 16 waves / column bytes) points per wave, rounded down to 8, at least
    8: every value 8 .. 64.  long16: on the last p at which 16 points fit (with 160 KB: p = 460, s = 75, where the division
    comes out at 16 exactly) and on the next (20 bytes short: 8); long8: the last p at which the 8 points fit that the
    screen asks for, and the next, where the call must take the all-exact kernels.  n leaves the last wave of the last
    work item with fewer points than it stages."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    p, s, no_rec, path, pts = _stage_case(L, name)
    assert fits_screen(L, p)
    n, K = 3001, 20
    gam = s / p
    X, big, cols = spiked(random_csc(p, n, s, seed=p + s))
    Cm = spiked_centres(np.random.default_rng(s), p, K, gam, big)
    if no_rec:
        set_switch(monkeypatch, gpu_ctx, "SPKM_NO_REC")
    eng = LloydEngine(make_shard(gpu_ctx, X), K, gam)
    for it in range(2):                                      # (the second call: carried bounds, kept sort)
        eng.assign_accumulate_step(dev_centres(gpu_ctx, Cm))
        torch.cuda.synchronize()
        t = eng.last_assign_tile()
        assert eng.last_path_info()[0] == path and t[3] == pts, (name, p, s, t, eng.last_path_info())
        ra, _ = held(eng, oracle, X, Cm, gam, tag=f"staged {name} p={p} s={s} call {it}")
        assert np.all(ra[cols] == K - 1)
        Cm = Cm * (1 + 1e-9)


@pytest.mark.parametrize("name", ["tier64", "tier48", "tier32", "tier16", "edge-fits", "edge-over"])
def test_single_centre_stream_stages_every_number_of_points_per_wave(gpu_ctx, oracle, name):
    """spkm_assign_dev with K = 1 (the k-means++ rounds): k_exact_dist1 with 16 .. 64 staged points per wave, on the last
    p at which 16 fit (s = 64) and on the next, where the call falls through to the tiled / generic kernels."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    if name.startswith("tier"):
        t, p = int(name[4:]), 500
        s = next(s for s in range(64, 0, -1) if fits_k1(L, p, s) and k1_pts(L, p, s) == t)
    else:
        s = 64
        p = edge(lambda q: fits_k1(L, q, s), name[5:])
    stream = fits_k1(L, p, s)
    n = 2501
    gam = s / p
    X, big, cols = spiked(random_csc(p, n, s, seed=p + s))
    Cm = spiked_centres(np.random.default_rng(s), p, 1, gam, big)
    eng = LloydEngine(make_shard(gpu_ctx, X), 1, gam)
    eng.assign_step(dev_centres(gpu_ctx, Cm))
    torch.cuda.synchronize()
    t = eng.last_assign_tile()
    assert t[3] == (k1_pts(L, p, s) if stream else 0) and t[0] == (0 if stream else pick_kt(L, p, 1)), (name, p, s, t)
    ra, rd = oracle.assign(p, n, *parts(X), Cm, gam)
    assert not eng.assign.any().item() and not ra.any()
    assert np.array_equal(eng.mind.cpu().numpy(), rd)
    st = eng.stats.cpu().numpy()
    assert abs(st[0] - np.sum(rd * rd)) <= 1e-12 * np.sum(rd * rd) and st[1] == rd.max() and int(st[2]) == int(np.argmax(rd))
    assert eng.nk.cpu().numpy().tolist() == [n]


# ---- e. sorted against atomic accumulation; streaming against generic distances ----
@pytest.mark.parametrize("K", [3, 300])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("side", SIDES)
def test_accumulation_on_both_sides_of_the_slab_limit(gpu_ctx, oracle, side, ragged, K):
    """spkm_accumulate_dev: k_accumulate_sorted keeps a cluster's sums and counts in a 12 B x p slab of at most 64 KB;
    beyond it k_accumulate_atomic.  K = 300: k_plan_segments strides over the clusters past 256; cluster 1 is empty."""
    from sparsifiedkmeans_amd.engine import LloydEngine

    L = lds_of(gpu_ctx)
    p = edge(lambda q: fits_slab(L, q), side)
    s, n = 12, 2000
    gam = s / p
    X, big, cols = spiked(random_csc(p, n, s, seed=p + K, ragged=ragged, empty_cols=(5,) if ragged else ()))
    Cm = spiked_centres(np.random.default_rng(K), p, K, gam, big)
    Cm[:, 1] = gam * 1e3                                      # far from everything: an empty cluster
    eng = LloydEngine(make_shard(gpu_ctx, X), K, gam)
    assert eng.shard.ir_bits == 16
    eng.assign_step(dev_centres(gpu_ctx, Cm))
    eng.accumulate_step()
    torch.cuda.synchronize()
    t = eng.last_assign_tile()
    assert t[4] == (1 if side == "fits" else 2) and t[0] == pick_kt(L, p, K), t
    ra, _ = held(eng, oracle, X, Cm, gam, stats=True, centres=True, tag=f"slab p={p} K={K} ragged={ragged}")
    assert not np.any(ra == 1) and np.all(ra[cols] == K - 1)


@pytest.mark.parametrize("side", SIDES)
def test_distances_on_both_sides_of_the_streaming_limit(gpu_ctx, oracle, side):
    """spkm_distances_stats_dev on a shard that has the record layout (here: only the record layout): the streaming
    record kernel while centroid, slab and 16 x 16 staged points of 64 entries fit, the generic kernel beyond"""
    from sparsifiedkmeans_amd.engine import LloydEngine, Shard, record_bytes

    L = lds_of(gpu_ctx)
    s, n, K = 64, 2003, 7
    p = edge(lambda q: fits_pipe(L, q, s), side)
    gam = s / p
    X, big, cols = spiked(random_csc(p, n, s, seed=p))
    R = record_bytes(s, 16)
    rec = np.zeros((n, R), np.uint8)
    rec[:, :8 * s] = X.data.reshape(n, s).view(np.uint8)
    rec[:, 8 * s:10 * s] = X.indices.astype(np.uint16).reshape(n, s).view(np.uint8)
    buf = torch.zeros(n * R + 256, dtype=torch.uint8, device=f"cuda:{gpu_ctx.device}")
    buf[:n * R] = torch.tensor(rec.ravel(), device=buf.device)
    eng = LloydEngine(Shard.from_records(gpu_ctx, p, n, s, buf), K, gam)
    Cm = spiked_centres(np.random.default_rng(3), p, K, gam, big)
    c = dev_centres(gpu_ctx, Cm)
    eng.assign_accumulate_step(c)
    torch.cuda.synchronize()
    ra, rd = held(eng, oracle, X, Cm, gam, tag=f"records p={p}")
    assert np.all(ra[cols] == K - 1)
    eng.mind.zero_()
    eng.stats.zero_()
    eng.distances(c)
    torch.cuda.synchronize()
    assert eng.last_assign_tile()[5] == (1 if side == "fits" else 2), eng.last_assign_tile()
    assert np.array_equal(eng.mind.cpu().numpy(), rd)
    st = eng.stats.cpu().numpy()
    assert abs(st[0] - np.sum(rd * rd)) <= 1e-12 * np.sum(rd * rd) and st[1] == rd.max() and int(st[2]) == int(np.argmax(rd))
