"""Worker of tests/test_gpu_consensus.py::test_every_case_again_under_debug_poison: the library reads FALCON_DEBUG_POISON once
per process, so the cases (the designed ones of
tests/test_gpu_consensus_edges.py and its lds_turns included) run again in a fresh process that has it set.  Never imported by pytest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("FALCON_DEBUG_POISON") == "1"
    from falcon_amd.device import Context
    from tests import test_gpu_consensus as t
    ctx = Context(0)
    for name in t.CASES:
        t.check_case(ctx, name)
        print("ok", name, flush=True)
    t.check_second_call_and_permutation(ctx)
    t.check_undersized_cap(ctx)
    from tests import consensus_cases as cc
    from tests import test_gpu_consensus_edges as e
    for name in cc.DECISION_CASES:
        e.check_decision_case(ctx, name)
        print("ok", name, flush=True)
    e.check_turn_case(ctx, "lds_turns")
    print("ok lds_turns", flush=True)
    print("poison ok", flush=True)


if __name__ == "__main__":
    main()
