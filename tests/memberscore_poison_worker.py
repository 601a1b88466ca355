"""Worker of tests/test_gpu_memberscore.py::test_template_case_again_under_debug_poison: the library reads FALCON_DEBUG_POISON
once per process, so the cases run again in a fresh process that has it set.  Never imported by pytest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("FALCON_DEBUG_POISON") == "1"
    from falcon_amd.device import Context
    from tests import memberscore_cases as mc
    from tests import test_gpu_memberscore as t
    ctx = Context(0)
    # a small call first: the larger ones after it grow the unit's slots and the sort's scratch
    case, tol = mc.tile_case(63, "interleaved")
    t.check(ctx, case, *mc.medoid_form(case), tol)
    print("ok tile", flush=True)
    t.check_template(ctx)
    print("ok template", flush=True)
    case, rep, rep_row, tol = mc.big_rep_case()
    t.check(ctx, case, rep, rep_row, tol)
    print("ok big representative", flush=True)
    t.test_summary_sizes_on_the_device(ctx)
    print("poison ok", flush=True)


if __name__ == "__main__":
    main()
