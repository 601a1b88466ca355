"""Worker of tests/test_gpu_msp.py::test_every_check_again_under_debug_poison: the library reads FALCON_DEBUG_POISON once per
process, so the ABI-level checks run again in a fresh process that has it set.  Never imported by pytest."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("FALCON_DEBUG_POISON") == "1"
    from falcon_amd.device import Context
    from tests import test_gpu_msp as t
    ctx = Context(0)
    t.run_all(ctx)
    print("poison ok", flush=True)


if __name__ == "__main__":
    main()
