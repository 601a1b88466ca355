"""Worker of tests/test_gpu_front_shapes.py::test_front_kernels_again_under_debug_poison: the library reads FALCON_DEBUG_POISON
once per process, so the cases run again in a fresh process that has it set.  Never imported by pytest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("FALCON_DEBUG_POISON") == "1"
    from falcon_amd.device import Context
    from tests import test_gpu_front_shapes as t
    from tests import test_gpu_preprocess as tp
    from tests import test_gpu_rescore as tr
    ctx = Context(0)
    cus = t.device_cus()
    # a small call first: the larger ones after it grow `fal_process_spectra`'s three slots and the scan's
    t.check_small_prep(ctx)
    print("ok five spectra", flush=True)
    t.check_edge_table(ctx)
    print("ok edge table", flush=True)
    tp.test_process_spectra_long_and_degenerate(ctx)
    print("ok 20,000 peaks", flush=True)
    for mode in ("f32", "f16+image"):
        t.check_vectorize(ctx, cus, 2, 50, 64, mode, True)
    print("ok vectorize chunk 2", flush=True)
    tr.test_rescore_matches_reference_cosine_fast_golden(ctx)
    print("poison ok", flush=True)


if __name__ == "__main__":
    main()
