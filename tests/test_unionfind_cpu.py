"""csrc/unionfind.h without a GPU: tests/hostbuild_unionfind.py's program -- eight threads racing the header's union, final
find and root store on deep chains, stars, two interleaved chains, a random graph and the smallest graphs, against a sequential
union-find of its own -- as a child process with nothing set in its environment; once under ThreadSanitizer, once plain."""
import subprocess

import pytest

from tests import hostbuild_unionfind as hb

pytestmark = pytest.mark.skipif(hb.plain_compiler() is None,
                                reason="no plain host C++ compiler (hipcc's host side takes the header's device form)")


def _run_and_check(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stderr == "", r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["ok " + g for g in hb.GRAPHS], lines


def test_eight_threads_race_the_header_clean_under_threadsanitizer(tmp_path):
    why = hb.sanitizer_missing(tmp_path)
    if why:
        pytest.skip(why)
    _run_and_check(hb.build(tmp_path, "unionfind_tsan", hb.TSAN))


def test_eight_threads_race_the_header_without_the_sanitizer(tmp_path):
    _run_and_check(hb.build(tmp_path, "unionfind_plain", hb.PLAIN))
