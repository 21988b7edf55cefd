"""CPU: the plan harness itself (tests/plan_harness.py over tests/native/plan_harness.cpp).  The tests of policy.h reach its
structs by field name only, so what has to hold is that no name is silently missing or misread: an unknown name raises, every
field of spkm_call_in holds what was written to it and nothing else does, and the plan's field list -- read from the harness,
whose build fails when it does not name every member of the struct -- has every name the test modules read."""
import glob
import os
import re

import pytest

import plan_harness as PH

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("call_in", "call_plan", "mover_plan", "mover2_plan", "policy")


def test_an_unknown_name_raises():
    for kind in KINDS:
        s = PH.Struct(kind)
        with pytest.raises(KeyError):
            s.set(no_such_field=1)
        with pytest.raises(KeyError):
            s.get("no_such_field")
    for make in (PH.call_in, PH.policy):
        with pytest.raises(KeyError):
            make(no_such_field=1)
    with pytest.raises(KeyError):
        PH.call_in(flags=["no_such_flag"])
    with pytest.raises(KeyError):
        PH.Struct("no_such_struct")
    with pytest.raises(KeyError):
        PH.fields("no_such_struct")
    with pytest.raises(KeyError):
        PH.const("no_such_constant")
    with pytest.raises(KeyError):
        PH.observe(PH.policy(), 1000.0, 1, 13, no_such_counter=1)
    with pytest.raises(KeyError):
        PH.plan(PH.call_in(n=1, K=2, fixed_s=4), PH.policy())["no_such_field"]
    with pytest.raises(KeyError):
        PH.plan(PH.call_in(n=1, K=2, fixed_s=4), PH.policy()).no_such_field


def test_every_input_field_holds_what_was_written_to_it():
    names = PH.fields("call_in")
    assert len(names) == len(set(names)) == 40
    fresh = PH.Struct("call_in").read()
    bools = [f for f in names if PH.Struct("call_in", **{f: 7}).get(f) == 1]          # (a bool keeps 7 as true)
    assert len(bools) == 28 and all(fresh[f] == 0 for f in bools)
    # the numbers: all at once, each its own value
    want = {f: 1000 + 17 * j for j, f in enumerate(names) if f not in bools}
    s = PH.Struct("call_in", **want)
    got = s.read()
    assert {f: got[f] for f in want} == want and all(got[f] == 0 for f in bools)
    assert all(s.get(f) == v for f, v in want.items())
    # the bools: one at a time, and no other field moves
    for f in bools:
        got = PH.Struct("call_in", **want, **{f: True}).read()
        assert got == dict(want, **{b: int(b == f) for b in bools}), f
    # wide values arrive whole
    big = PH.Struct("call_in", n=1 << 40, sp_blocks=(1 << 40) + 1, lds_max=1 << 33).read()
    assert (big.n, big.sp_blocks, big.lds_max) == (1 << 40, (1 << 40) + 1, 1 << 33)
    assert PH.policy(last_movers=1 << 40, ev_cum_movers=(1 << 41) + 3).read() == dict(
        PH.policy().read(), last_movers=1 << 40, ev_cum_movers=(1 << 41) + 3)


def test_the_plan_field_list_has_every_name_the_modules_read():
    import test_bounds_plan as B
    import test_far_bounds_plan as FB
    import test_far_events_plan as FE
    import test_far_ragged_plan as FR

    plan = PH.plan_fields()
    assert len(plan) == len(set(plan)) == 37
    assert plan[:4] == ("G", "pl_last", "Gs", "nr") and plan[-2:] == ("ev_cap", "seg_ev")      # (declaration order: the golden file's columns)
    for kind in KINDS:
        assert len(PH.fields(kind)) == len(set(PH.fields(kind))), kind
    # the modules' lists of plan fields, and of input flags
    for name in B.ON + FB.NEVER + FE.MAY + FE.NEVER:
        assert name in plan, name
    for name in B.IN_FLAGS + FB.IN_FLAGS + FB.BAIT + FE.IN_FLAGS + FE.ON + FR.IN_FLAGS + FR.ON:
        assert PH.ALIASES.get(name, name) in PH.fields("call_in"), name
    assert set(PH.ALIASES.values()) <= set(PH.fields("call_in"))
    # every field a module reads with a literal: d["name"] in the plan modules (mover plans included; test_mover2_plan.py
    # subscripts its ARGS with "K" too), .name on a plan in test_policy.py
    known = set(plan) | set(PH.fields("mover_plan")) | set(PH.fields("mover2_plan")) | {"K"}
    read = set()
    for path in glob.glob(os.path.join(HERE, "test_*plan*.py")):
        if os.path.basename(path) != "test_plan_harness.py":
            read |= set(re.findall(r'\w\["(\w+)"\]', open(path).read()))
    src = open(os.path.join(HERE, "test_policy.py")).read()
    read |= {a or b for a, b in re.findall(r"\bpl\.(\w+)|\.plan\([^()]*\)\.(\w+)", src)}
    assert len(read) > 40 and read <= known, sorted(read - known)
