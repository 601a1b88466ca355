"""`fal_consensus_spectra` at its decisions and at the sizes where its grids turn, bit for bit against the numpy restatement
(tests/consensus_cases.py, where every case and the witness that it reaches its target are defined; tests/test_consensus_cpu.py
asserts the witnesses without a GPU):
  * the decision cases: the gap rule at, one ulp above and across a doubling of the ulp of the tolerance; the quorum where the
    double product rounds; groups without weight; intensities whose squares leave float32; the pooled order made visible by
    signed intensities on both sort paths; labels and medoids that name nothing; the bitonic padding sizes; group starts around
    the emit kernel's 64-lane chunks; clusters above the LDS cut at the first and last id;
  * `lds_turns`: every workgroup of cons_sort_lds_kernel sorts a second cluster, thirteen a third, and the emit waves turn;
  * `flat_turns`: every flat kernel's grid-stride loop turns -- over rows, clusters, pooled peaks and device-wide-sort peaks.
The turn sizes follow from the device's CU count; their expected output is gathered from a library of clusters."""
import functools

import numpy as np
import pytest

from tests import consensus_cases as cc
from tests.test_gpu_consensus import _equal, _gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from falcon_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def device_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _run(ctx, part, tol, q, ref):
    """the call with room for the expected output (a cluster that falls back to a row of another cluster repeats its peaks)"""
    got = _gpu(ctx, part, tol, q, nnz_cap=max(len(part["mz"]), int(ref[0][-1])))
    _equal(got, ref, part)
    return got


@functools.lru_cache(maxsize=None)
def _decision(name):
    case = cc.DECISION_CASES[name]()
    p = case["part"]
    ref = cc.consensus_reference(p["mz"], p["intensity"], p["indptr"], p["labels"], p["medoids"], case["tol"], case["q"])
    case["witness"](ref)
    return case, ref


def check_decision_case(ctx, name):
    from falcon_amd import _lib
    assert cc.CUT == _lib.CONS_LDS_PEAKS
    case, ref = _decision(name)
    return _run(ctx, case["part"], case["tol"], case["q"], ref)


@functools.lru_cache(maxsize=None)
def _turn_case(which, cus):
    builder, library = {"lds_turns": (cc.lds_turns, cc.lds_turns_library), "flat_turns": (cc.flat_turns, cc.flat_turns_library)}[which]
    part, pick, cond = builder(cus)
    lib = library()[0]
    lib_ref = cc.consensus_reference(lib["mz"], lib["intensity"], lib["indptr"], lib["labels"], lib["medoids"], 0.05, 0.25)
    return part, cond, cc.gather_expected(lib_ref, pick)


def check_turn_case(ctx, which):
    part, cond, ref = _turn_case(which, device_cus())
    assert all(cond.values()), cond                                 # the grids of THIS device turn
    return _run(ctx, part, 0.05, 0.25, ref)


@pytest.mark.parametrize("name", list(cc.DECISION_CASES))
def test_decision_case_equals_the_restatement_bit_for_bit(ctx, name):
    got = check_decision_case(ctx, name)
    if name.startswith("big_ids") or name == "chain_order":
        assert (got[3] & cc.GLOBAL).any()


def test_lds_sort_workgroups_take_a_second_and_a_third_cluster(ctx):
    got = check_turn_case(ctx, "lds_turns")
    assert not (got[3] & cc.GLOBAL).any()


def test_flat_kernels_take_a_second_grid_turn(ctx):
    got = check_turn_case(ctx, "flat_turns")
    assert ((got[3] & cc.GLOBAL) != 0).sum() > 1
