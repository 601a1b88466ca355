"""Worker of tests/test_gpu_network.py::test_cases_again_under_debug_poison: the library reads FALCON_DEBUG_POISON once per
process, so the cases run again in a fresh process that has it set.  Never imported by pytest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("FALCON_DEBUG_POISON") == "1"
    from falcon_amd.device import Context
    from tests import network_cases as nc
    from tests import test_gpu_network as t
    ctx = Context(0)
    # a small call first: the larger ones after it grow the unit's slots and the sorts' scratch
    t.check_tile(ctx, 2, "all")
    for n, band in ((63, "equal"), (65, "mid"), (130, "all"), (64, "all")):
        t.check_tile(ctx, n, band)
    print("ok tiles", flush=True)
    nodes = nc.analogue_case()
    analogue = (nodes, nc.score_pairs(nodes, nc.ANALOGUE["fragment_tol"], nc.ANALOGUE["max_shift"]))
    for top_k in (5, 0, 1):
        t.check_analogue(ctx, analogue, top_k)
    print("ok analogue", flush=True)
    t.check_large(ctx)
    print("ok large sides", flush=True)
    t.check_tile(ctx, 1, "all")
    print("poison ok", flush=True)


if __name__ == "__main__":
    main()
