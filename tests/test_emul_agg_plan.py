"""CPU tier: the aggregation plan (adcensus_amd/csrc/agg_plan.h, compiled alone under g++ by tests/emul/emul_agg_plan.cpp).

tests/golden/agg_plan_table.txt holds what the launcher launched before it was split into a plan and an executor: per scenario the
inputs (S line) and the SHA-256 of its log -- every kernel launch with its name, grid, block, LDS bytes and arguments (L lines), the
profiling events (E) and the state of the handle afterwards (R) -- and, for 22 scenarios, that log in full.  The driver writes
every scenario's plan out in the same format; it must equal the record line for line: kernel and template flags, ring depth,
geometry, grid, LDS, gate, volumes, the k_agg_apply behind a sparse launch, the label, the counters and the end volume.  The second
test checks the invariants of a plan over randomly drawn inputs and switches (fixed seeds)."""
import hashlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "agg_plan_table.txt")


@pytest.fixture(scope="module")
def emul_agg_plan():
    out_dir = os.path.join(ROOT, "tests", "emul", "_build")
    exe = os.path.join(out_dir, "emul_agg_plan")
    deps = [os.path.join(ROOT, "tests", "emul", "emul_agg_plan.cpp"), os.path.join(ROOT, "adcensus_amd", "csrc", "agg_plan.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        os.makedirs(out_dir, exist_ok=True)
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", deps[0], "-o", exe])
    return exe


def _blocks(lines):
    """{scenario: [lines behind its S line]} of a text whose scenarios start with an S line"""
    out, cur = {}, None
    for line in lines:
        if line.startswith("S "):
            cur = line.split()[1]
            assert cur not in out, cur
            out[cur] = []
        elif cur is not None and not line.startswith(("#", "D ")):
            out[cur].append(line)
    return out


FORMS = ("k_agg_march<false,false,false,", "k_agg_march<false,false,true,true,false,1,", "k_agg_march<true,true,true,false,true,2,false>",
         "k_agg_march<true,true,true,false,true,2,true>", "k_agg_gather<", "k_agg_regring<", "k_agg_regring_pair<", "k_agg_regring_cost", "k_agg_rr2<",
         "k_agg_rr2_cost", "k_cost_agg_flat", "k_agg_apply<")


def test_plan_equals_the_recorded_launches(emul_agg_plan):
    text = open(TABLE).read().splitlines()
    want_sha = {l.split()[1]: l.rsplit("sha256=", 1)[1] for l in text if l.startswith("S ")}
    full = {name: log for name, log in _blocks(text).items() if log}
    plans = _blocks(subprocess.check_output([emul_agg_plan, "table", TABLE], text=True).splitlines())
    assert len(want_sha) >= 500 and len(full) >= 20 and set(plans) == set(want_sha)
    for name, log in full.items():  # the scenarios whose log is in the table: line for line, and the table's own hash
        assert plans[name] == log, name
        assert hashlib.sha256("".join(l + "\n" for l in log).encode()).hexdigest() == want_sha[name], name
    wrong = [name for name, lines in plans.items() if hashlib.sha256("".join(l + "\n" for l in lines).encode()).hexdigest() != want_sha[name]]
    assert not wrong, wrong
    kernels = {l.split()[1] for lines in plans.values() for l in lines if l.startswith("L ")}
    for f in FORMS:  # every form of AggForm (and k_agg_apply) appears in the table
        assert any(k.startswith(f) for k in kernels), f


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_plan_invariants_on_random_inputs(emul_agg_plan, seed):
    r = subprocess.run([emul_agg_plan, "random", str(seed), "4000"], capture_output=True, text=True)
    assert r.returncode == 0 and "violations=0" in r.stdout, r.stdout
    assert int(re.search(r"two_plan=(\d+)", r.stdout).group(1)) > 100  # (the two-plan invariants were exercised)
