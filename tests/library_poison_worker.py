"""Worker of tests/test_gpu_library.py::test_cases_again_under_debug_poison: the library reads FALCON_DEBUG_POISON once per
process, so the cases run again in a fresh process that has it set.  Never imported by pytest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("FALCON_DEBUG_POISON") == "1"
    from falcon_amd.device import Context
    from tests import library_cases as lc
    from tests import test_gpu_library as t
    ctx = Context(0)
    # a small call first: the larger ones after it grow the unit's slots and the sorts' scratch
    t.check_tile(ctx, 1, 1, "all")
    for nq, nl, band in ((63, 64, "equal"), (65, 130, "mid"), (130, 65, "all"), (64, 64, "all")):
        t.check_tile(ctx, nq, nl, band)
    print("ok tiles", flush=True)
    q, l = lc.analogue_case()
    r = lc.rule(True, max_shift=lc.ANALOGUE["max_shift"])
    analogue = (q, l, r, lc.score_pairs(q, l, lc.ANALOGUE["fragment_tol"], r))
    for top_n in (3, 0, 1):
        t.check_analogue(ctx, analogue, top_n)
    print("ok analogue", flush=True)
    t.check_large(ctx)
    print("ok large sides", flush=True)
    t.check_tile(ctx, 1, 64, "all")
    print("poison ok", flush=True)


if __name__ == "__main__":
    main()
