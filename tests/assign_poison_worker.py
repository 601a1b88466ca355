"""Worker of tests/test_gpu_assign.py::test_template_case_again_under_debug_poison: the library reads FALCON_DEBUG_POISON once
per process, so the cases run again in a fresh process that has it set.  Never imported by pytest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("FALCON_DEBUG_POISON") == "1"
    from falcon_amd.device import Context
    from tests import assign_cases as ac
    from tests import test_gpu_assign as t
    ctx = Context(0)
    # the library side larger than the query side: the second sort of the call grows the sort's scratch
    t.check(ctx, *ac.ladder_case(63, 200), 20.0, "ppm", None, 0.05, 0)
    print("ok ladder", flush=True)
    q, l = ac.template_split()
    t.check(ctx, q, l, *ac.TEMPLATE_PARAMS["da005"])
    print("ok template", flush=True)
    t.check(ctx, *ac.ladder_case(10, 0), 20.0, "ppm", None, 0.05, 0)
    print("poison ok", flush=True)


if __name__ == "__main__":
    main()
