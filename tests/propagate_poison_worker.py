"""Worker of tests/test_gpu_propagate.py::test_cases_again_under_debug_poison: the library reads FALCON_DEBUG_POISON once per
process, so the cases run again in a fresh process that has it set.  Never imported by pytest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("FALCON_DEBUG_POISON") == "1"
    from falcon_amd.device import Context
    from tests import propagate_cases as pc
    from tests import test_gpu_propagate as t
    ctx = Context(0)
    # a small call first: the larger ones after it grow the unit's slot
    t.check_case(ctx, "two-seeds-tie")
    for name in sorted(pc.CASES, key=lambda k: pc.CASES[k][0]["n"]):
        t.check_case(ctx, name)
    print("ok cases", flush=True)
    t.check_case(ctx, "no-links")
    for name, (g, seed, max_hops, min_score) in sorted(pc.invalid_cases().items()):
        rc, out, _, _ = t.raw_call(ctx, g, seed, max_hops, min_score)
        assert rc == -1 and all((o == t.MARK).all() for o in out), name
    t.check_case(ctx, "random-5000")
    print("poison ok", flush=True)


if __name__ == "__main__":
    main()
