"""The one loader of tests/native/plan_harness.cpp -- a C face on sparsifiedkmeans_amd/csrc/policy.h -- and the one way the
CPU tests state a fused call and read its plan.

 * lib(): the harness compiled with g++, once per process, every argtypes / restype set here;
 * Struct: a policy.h struct inside the harness, its fields set and read by name (an unknown name raises KeyError);
   call_in(...), policy(...) make the two a plan starts from, by keyword;
 * plan(inp, pol, ...): a plan made in the library's stages -- spkm_plan_tiles, spkm_plan_call, the device's refusals, and
   spkm_plan_sums when `rec` is given (run_screen's order; run_far stops after spkm_plan_call: rec=None) -- as a dict keyed by
   field name, in policy.h's declaration order (plan_fields());
 * the policy's methods by keyword (observe, launched), and the constants of policy.h by name (const)."""
import atexit
import ctypes as C
import functools
import os
import shutil
import subprocess
import tempfile
import weakref

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "native", "plan_harness.cpp")
FP, IP, LP = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_longlong)


@functools.lru_cache(maxsize=None)
def lib():
    tmp = tempfile.mkdtemp(prefix="plan_harness_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    so = os.path.join(tmp, "libplanharness.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", SOURCE, "-o", so])
    L = C.CDLL(so)
    i, ll, u64, dbl, s, h = C.c_int, C.c_longlong, C.c_uint64, C.c_double, C.c_char_p, C.c_void_p
    sig = {
        # structs by field name
        "ph_new": (h, [s]), "ph_free": (None, [s, h]), "ph_fields": (i, [s]), "ph_field_name": (s, [s, i]),
        "ph_get": (i, [s, h, s, LP]), "ph_set": (i, [s, h, s, ll]), "ph_get_all": (i, [s, h, LP]), "ph_const": (i, [s, LP]),
        # the plan's stages
        "plan_tiles": (None, [h, h, i]), "plan_call": (None, [h, h, h]), "plan_lose_events": (None, [h]),
        "plan_lose_pair": (None, [h]), "plan_sums": (None, [h, h, h, i]), "plan_movers": (None, [h, h, h, i, i]),
        "plan_movers2": (None, [h, h, h, i, i]),
        # spkm_policy's methods
        "pol_reset": (None, [h]), "pol_observe": (None, [h, dbl, i, i] + [dbl] * 9 + [i, dbl, i]), "pol_next": (None, [h, i, i, i, IP]),
        "pol_take_hinted_split": (i, [h, i, i]), "pol_launched": (None, [h] + [i] * 8), "pol_few_movers": (i, [h, dbl, i]),
        "pol_refresh_due": (i, [h, dbl]), "pol_form_on_device": (i, [h]), "pol_events_direct": (i, [h]),
        "pol_sums_by_events": (None, [h]), "pol_sums_by_full_pass": (None, [h]), "pol_event_cap": (u64, [u64, i]),
        # the free functions
        "pol_quad_split": (i, [i, i]), "pol_quad_split_late": (i, [i, i]), "pol_seg_points": (i, [ll, i]),
        "wide_kt": (i, [ll, u64]), "screen_quad": (i, [i, i]),
        "screen_width": (i, [ll, i, i, u64, u64, u64, i, i, i]), "far_screen": (i, [ll, i, i, u64, u64, u64, i, i, i, i]),
        "far_screen_ragged": (i, [ll, i, i, u64, u64, u64, i, i, i, i]), "tile_screen_ragged": (i, [ll, i, i, u64, u64, u64, i, i, i]),
        "exact_tile_fits": (i, [ll, u64]), "far_plane": (i, [i]), "far_planes": (i, [i, i]),
        "acc_form": (i, [ll, u64, i, i, IP]), "kpp_plan": (None, [ll, i, u64, C.c_uint, ll, u64, u64, IP]),
        "kpp_plan_ragged": (None, [ll, i, i, u64, u64, C.c_uint, ll, u64, u64, i, IP]),
        # the pick of the movers
        "mover_key": (u64, [C.c_float, i]), "pick_movers": (C.c_float, [FP, i, IP, IP]), "pick_movers2": (None, [FP, i, IP, IP, FP]),
        "pick_movers_threads": (C.c_float, [FP, i, i, C.c_float, IP, IP]),
        "pick_movers2_threads": (None, [FP, i, i, C.c_float, IP, IP, FP]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


@functools.lru_cache(maxsize=None)
def fields(kind):
    """the field names of a harness struct ("call_in", "call_plan", "mover_plan", "mover2_plan", "policy"), in its table's order"""
    n = lib().ph_fields(kind.encode())
    if n < 0:
        raise KeyError(f"the plan harness has no struct {kind!r}")
    return tuple(lib().ph_field_name(kind.encode(), j).decode() for j in range(n))


def plan_fields():
    """spkm_call_plan's field names in declaration order"""
    return fields("call_plan")


def const(name):
    """a constant of policy.h by its name there"""
    v = C.c_longlong()
    if lib().ph_const(name.encode(), C.byref(v)) != 0:
        raise KeyError(f"the plan harness knows no constant {name!r}")
    return v.value


class Fields(dict):
    """a struct read out: a dict keyed by field name (ints; a bool is 0 or 1) that also answers by attribute"""
    __getattr__ = dict.__getitem__


class Struct:
    """a policy.h struct that lives inside the harness; passes as the void* of the harness's functions"""

    def __init__(self, kind, **values):
        self.kind, self._k = kind, kind.encode()
        p = lib().ph_new(self._k)
        if not p:
            raise KeyError(f"the plan harness has no struct {kind!r}")
        self._as_parameter_ = C.c_void_p(p)
        weakref.finalize(self, lib().ph_free, self._k, self._as_parameter_)
        self.set(**values)

    def set(self, **values):
        for name, v in values.items():
            if lib().ph_set(self._k, self, name.encode(), int(v)) != 0:
                raise KeyError(f"{self.kind} has no field {name!r}")
        return self

    def get(self, name):
        v = C.c_longlong()
        if lib().ph_get(self._k, self, name.encode(), C.byref(v)) != 0:
            raise KeyError(f"{self.kind} has no field {name!r}")
        return v.value

    def read(self):
        names = fields(self.kind)
        out = (C.c_longlong * len(names))()
        lib().ph_get_all(self._k, self, out)
        return Fields(zip(names, out))


# ---- stating a call ----
# the short spellings of the modules' flag lists
ALIASES = {"carry": "carry_bounds", "synced": "assign_synced", "cl_stats": "cl_stats_valid", "force_pt": "force_point_list",
           "events": "far_events", "no_direct": "no_direct_events"}
# what the mover tile's tests hold fixed: gfx950's LDS and CUs, 64 teams, the block summaries of the previous call in place
# but counted over no blocks (with max_s = fixed_s, which the caller states)
MOVER_DEFAULTS = dict(lds_max=163840, num_cus=256, teams=64, same_assign=True, sp_clean=True, sp_blocks=0)


def sp_blocks_of(n):
    """the blocks the summaries of a shard of n points are kept over: npad / 1024 + 1"""
    return (n + 63) // 64 * 64 // 1024 + 1


def far_plane_of(K):
    """the plane width a far call's tiles are planned at"""
    return 64 if K <= 64 else (128 if K <= 128 else 256)


def call_in(flags=(), sp_blocks=None, **values):
    """spkm_call_in by keyword: every field not named keeps policy.h's default, but sp_blocks, which is sp_blocks_of(n)
    unless stated; `flags` names the bools to set (ALIASES allowed)"""
    values.update((ALIASES.get(f, f), True) for f in flags)
    return Struct("call_in", sp_blocks=sp_blocks_of(values.get("n", 0)) if sp_blocks is None else sp_blocks, **values)


def policy(**state):
    """a fresh spkm_policy with the named state set"""
    return Struct("policy", **state)


def policy_bits(bits, movers=0, ev_calls=0, ev_cum=0):
    """the policy state of the plan tables: bit 0 pt_next, bit 1 blocks_next, bit 2 movers_known; last_movers = movers;
    ev_calls / ev_cum: the refresh rule's counters"""
    return policy(pt_next=bits & 1, blocks_next=bits & 2, movers_known=bits & 4, last_movers=movers, ev_calls=ev_calls,
                  ev_cum_movers=ev_cum)


# ---- the plan, in the library's stages ----
def plan_struct(inp, pol, kt=None, lose=(), rec=None):
    """spkm_plan_tiles at kt centroids per tile (None: spkm_plan_kt), spkm_plan_call, the device's refusals in run_screen's
    order ("events": no event buffers; "pair_lds" / "ev_o": no pair plan LDS / pair buffer), then -- rec not None, as
    run_screen goes on and run_far does not -- spkm_plan_sums with or without the record layout"""
    L, pl = lib(), Struct("call_plan")
    L.plan_tiles(pl, inp, const("spkm_plan_kt") if kt is None else kt)
    L.plan_call(pl, inp, pol)
    if "events" in lose and pl.get("ev_possible"):
        L.plan_lose_events(pl)
    if ("pair_lds" in lose or "ev_o" in lose) and pl.get("pair_ev"):
        L.plan_lose_pair(pl)
    if rec is not None:
        L.plan_sums(pl, inp, pol, int(rec))
    return pl


def plan(inp, pol, kt=None, lose=(), rec=None):
    return plan_struct(inp, pol, kt, lose, rec).read()


def tile_plan(inp, kt):
    """spkm_plan_tiles alone"""
    pl = Struct("call_plan")
    lib().plan_tiles(pl, inp, kt)
    return pl.read()


def movers(inp, pl, K, sw):
    """spkm_plan_movers behind a plan made by plan_struct"""
    m = Struct("mover_plan")
    lib().plan_movers(m, inp, pl, K, sw)
    return m


def movers2(first, pl, K, sw):
    """spkm_plan_movers2 behind the first level's plan"""
    m = Struct("mover2_plan")
    lib().plan_movers2(m, first, pl, K, sw)
    return m


# ---- the policy's methods by keyword ----
COUNTERS = ("listed", "ambig", "early", "skipped", "kept", "movers", "msteps", "pairs2", "early2", "full_opened", "one_cluster_steps",
            "may_regroup")


def observe(pol, n, tiles, nr, **counters):
    """spkm_policy::observe with the named counters, every other one 0"""
    unknown = set(counters) - set(COUNTERS)
    if unknown:
        raise KeyError(f"spkm_policy_counters has no field {sorted(unknown)}")
    lib().pol_observe(pol, n, tiles, nr, *(counters.get(c, 0) for c in COUNTERS))


def launched(pol, rounds_all, rounds, hinted, late, skipping, movers_counted, by_events=False, both_forms=False):
    lib().pol_launched(pol, rounds_all, rounds, int(hinted), int(late), int(skipping), int(movers_counted), int(by_events), int(both_forms))


def observe_hinted(n, tiles, nr, late, **counters):
    """observe() of a hinted call that ran the bounds test and counted movers, on a policy with no late calls left; returns
    [hint_cooldown, hint_fail_streak, prune_next_a, hint_late, hint_late_left]"""
    pol = policy()
    launched(pol, lib().pol_quad_split(nr, 0), nr, True, late, True, True)
    pol.set(prune_pending_a=0)              # (a hinted call: its split is not the unconditional form's)
    pol.set(hint_late_left=0, hint_late=False)
    observe(pol, n, tiles, nr, **counters)
    return [pol.get(f) for f in ("hint_cooldown", "hint_fail_streak", "prune_next_a", "hint_late", "hint_late_left")]
