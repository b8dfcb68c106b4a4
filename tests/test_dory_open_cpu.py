"""CPU: the Dory evaluation proof of jolt_amd/dory_open.py in log space (tests/dory_open_model.py) -- the model verifier accepts honest runs and rejects a one-off
error in any single message element or in the claimed evaluation -- and the bindings of the entries that build an opening's state on the device."""
import copy
import os
import random
import re

import pytest

import dory_open_model as OM
from jolt_amd import ffi

R = OM.R
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SHAPES = [(0, 1), (1, 1), (2, 2), (1, 3), (2, 3), (3, 3), (4, 5)]


def instance(nu, sigma, seed):
    rng = random.Random(seed)
    n, rows = 1 << sigma, 1 << nu
    g1, g2 = [rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(n)]
    h1, h2 = rng.randrange(1, R), rng.randrange(1, R)
    matrix = [[rng.randrange(R) for _ in range(n)] for _ in range(rows)]
    left, right = [rng.randrange(R) for _ in range(rows)], [rng.randrange(R) for _ in range(n)]
    challenges = [(rng.randrange(1, R), rng.randrange(1, R)) for _ in range(sigma)]
    gamma, d = rng.randrange(1, R), rng.randrange(1, R)
    t_rows, commitment, v, y = OM.statement(g1, g2, matrix, left, right)
    proof = OM.prove(g1, g2, h1, h2, t_rows, v, left, right, challenges, gamma)
    check = lambda p, y_claimed=y: OM.verify(g1, g2, h1, h2, commitment, y_claimed, left, right, p, challenges, gamma, d)  # noqa: E731
    return dict(proof=proof, check=check, y=y, matrix=matrix, left=left, right=right, v=v)


@pytest.mark.parametrize("nu,sigma", SHAPES)
def test_the_model_verifier_accepts_honest_runs(nu, sigma):
    inst = instance(nu, sigma, 100 * nu + sigma)
    assert len(inst["proof"]["rounds"]) == sigma and inst["check"](inst["proof"])
    # y is the evaluation: L^T M R from the definition, not through v
    want = sum(inst["left"][i] * inst["matrix"][i][j] * inst["right"][j] for i in range(1 << nu) for j in range(1 << sigma)) % R
    assert inst["y"] == want


@pytest.mark.parametrize("nu,sigma", SHAPES)
def test_the_model_verifier_rejects_one_off_errors(nu, sigma):
    """+1 in C, D2, E1, in every element of every round's two messages, in w1, w2 and in y -- one at a time"""
    inst = instance(nu, sigma, 200 * nu + sigma)
    proof, check = inst["proof"], inst["check"]

    def tampered(edit):
        p = copy.deepcopy(proof)
        edit(p)
        return p

    def bump(t, j):
        return tuple((x + 1) % R if k == j else x for k, x in enumerate(t))

    for j in range(3):
        assert not check(tampered(lambda p: p.__setitem__("vmv", bump(p["vmv"], j)))), ("vmv", j)
    for r in range(sigma):
        for which in (0, 1):
            for j in range(6):
                def edit(p, r=r, which=which, j=j):
                    msgs = list(p["rounds"][r])
                    msgs[which] = bump(msgs[which], j)
                    p["rounds"][r] = tuple(msgs)
                assert not check(tampered(edit)), ("round", r, which, j)
    for j in range(2):
        assert not check(tampered(lambda p: p.__setitem__("final", bump(p["final"], j)))), ("final", j)
    assert not check(proof, (inst["y"] + 1) % R)
    assert check(proof)


NEW_ENTRIES = ["jolt_dory_state_alloc", "jolt_dory_state_from_table", "jolt_dory_state_combine_hints", "jolt_dory_state_fixed_base_mul"]
NEW_METHODS = ["dory_state_alloc", "dory_state_from_table", "dory_state_combine_hints", "dory_state_fixed_base_mul"]


def test_the_state_entries_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "jolt_hip.h")).read()
    binding = open(os.path.join(ROOT, "jolt_amd", "ffi.py")).read()
    rust = open(os.path.join(ROOT, "rust", "jolt-kernels-hip", "src", "ffi.rs")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint32_t\s+" + name + r"\s*\(", header), name
        assert hasattr(ffi.lib(), name), name
        assert f"lib().{name}(" in binding or f'_call("{name}", ' in binding, name
        assert f"pub fn {name}(" in rust, name
    for method in NEW_METHODS:
        assert callable(getattr(ffi.Context, method)), method


def test_the_opening_module_imports_without_a_gpu():
    from jolt_amd import dory_open
    from jolt_amd.dory_reduce import DoryReduce
    assert callable(DoryReduce.from_resident)
    for name in ("DorySetup", "DoryOpening", "dory_commit_tier2"):
        assert callable(getattr(dory_open, name)), name
    assert all(callable(getattr(dory_open.DoryOpening, m)) for m in ("vmv_message", "final_message", "build_state", "close"))
    assert "dory-pcs" in dory_open.__doc__  # the module says whose protocol it embodies and what stays unpinned

