"""The launch kinds of the 4-lanes-per-point screen (k_screen_quad, csrc/screen_quad.hip) that the fused call can reach,
as the host code selects them (csrc/policy.h, spkm_plan_call).  A plain helper for the tests, not a conftest:
tests/test_policy.py pins it against the compiled policy.h, tests/test_gpu_screen_forms.py checks that a case reaches
every kind it lists.

A launch kind is (pts, nr, rounds_all, hinted):
    pts         the list names points (point-granular carried bounds) rather than 16-point steps or all points;
    nr          rounds of 4 entries per column, ceil(s / 4), 1 ..= 16;
    rounds_all  rounds evaluated for all centroids (nr: the plain form; fewer: a two-phase form with that split);
    hinted      the two-phase form compares the partial sums with per-point hints (a_hint != nullptr).
What a call ran is read back as (spkm_last_screen_rounds()[0], [1], last_screen_mode()[7] == 2, last_screen_mode()[0] == 2)."""

NR_MAX = 16


def split_early(nr: int, pts: bool = False) -> int:
    """policy.h, quad_split"""
    if nr < 3:
        return nr
    if pts:
        return max((nr + 2) // 4, 2)
    return max(nr // 8, 1)


def split_late(nr: int, pts: bool = False) -> int:
    """policy.h, quad_split_late (0: none)"""
    if pts:
        return (nr + 1) // 2 if nr >= 10 else 0
    return max((nr + 2) // 4, 2) if nr >= 6 else 0


def unconditional_split(nr: int, pts: bool) -> int:
    """rounds for all centroids of the unconditional two-phase form (policy.h, spkm_plan_call): the late split of the step-major copy
    where it has one, else the early one; the point-list kernels take their early split"""
    if not pts and split_late(nr) > 0:
        return split_late(nr)
    return split_early(nr, pts)


def expected_kinds(nr: int, pts: bool) -> dict:
    """{name: (pts, nr, rounds_all, hinted)} of every kind reachable for this round count and list kind"""
    kinds = {"plain": (pts, nr, nr, False)}
    a = unconditional_split(nr, pts)
    if a < nr:
        kinds["two-phase"] = (pts, nr, a, False)
    e = split_early(nr, pts)
    if e < nr:
        kinds["hinted-early"] = (pts, nr, e, True)
        late = split_late(nr, pts)
        if late > e:
            kinds["hinted-late"] = (pts, nr, late, True)
    return kinds


def all_kinds() -> set:
    """every reachable launch kind of one row-id width"""
    return {k for nr in range(1, NR_MAX + 1) for pts in (False, True) for k in expected_kinds(nr, pts).values()}


def compiled_form(pts: bool, nr: int, rounds_all: int) -> int:
    """TWO of the k_screen_quad instantiation that screen_quad.hip's dispatcher returns: 0 plain, 1 early split, 2 late"""
    if rounds_all >= nr:
        return 0
    return 2 if split_late(nr, pts) > 0 and rounds_all == split_late(nr, pts) else 1


def all_kernels() -> set:
    """(pts, nr, TWO) of every instantiation a reachable kind runs"""
    return {(k[0], k[1], compiled_form(k[0], k[1], k[2])) for k in all_kinds()}


def last_tile_body(K: int, p: int = 256, lds_max: int = 160 * 1024) -> int:
    """pl of the last centroid tile (policy.h, spkm_plan_tiles): 1 / 2 centroid pairs per lane for a narrow tile of <= 8 / <= 16,
    4 for a full one, 5 when <= 4 centroids are carried by the tile before"""
    G = (K + 31) // 32
    k_last = K - (G - 1) * 32
    pl = 1 if k_last <= 8 else (2 if k_last <= 16 else 4)
    if G >= 2 and k_last <= 4 and (p + 1) * (32 * 4 + 16) + 16 <= lds_max:
        pl = 5
    return pl
