"""Member scores and cluster summary without a GPU: the host build of csrc/memberscore.h against the numpy restatement
(tests/memberscore_cases.py), `summary_io`'s bytes for hand-written columns, and the option's place in `config`."""
import io

import numpy as np
import pytest

from tests import hostbuild_memberscore as hb
from tests import memberscore_cases as mc

needs_compiler = pytest.mark.skipif(not hb.have_compiler(), reason="no host C++ compiler")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return hb.build(tmp_path_factory.mktemp("memberscore_host"))


# ---- the header ----------------------------------------------------------------------------------------------------------------
@needs_compiler
def test_the_chains_of_the_sum_are_the_restatements(lib):
    assert lib.t_chains() == mc.CHAINS


@needs_compiler
def test_summary_fold_order_ties_and_sizes(lib):
    """sizes 1, 2, 64, 65, 5,000 (and an empty cluster), similarities over 2^-30 .. 1 with ties of the minimum, rows interleaved"""
    labels, sim, pmz, rt = mc.summary_case(mc.SUMMARY_SIZES, seed=4)
    want = mc.summary_ref(labels, len(mc.SUMMARY_SIZES), sim, pmz, rt)
    got = hb.summary(lib, labels, len(mc.SUMMARY_SIZES), sim, pmz, rt)
    for k in mc.COLUMNS:
        assert mc.same(got[k], want[k]), k
    assert list(want["size"]) == mc.SUMMARY_SIZES and want["worst_row"][5] == -1
    # the inputs do what they are for: the minimum is tied, the lowest row wins
    big = np.flatnonzero(labels == 4)
    assert np.sum(sim[big] == sim[big].min()) >= 2 and want["worst_row"][4] == big[np.argmin(sim[big])]


@needs_compiler
def test_the_sum_order_is_visible_in_the_bits(lib):
    """the plain row-order chain of the 5,000 similarities differs from the stated order's sum: a kernel that summed in another
    order would not pass the comparison"""
    labels, sim, pmz, _ = mc.summary_case([5000], seed=7, interleave=False)
    got = hb.summary(lib, labels, 1, sim, pmz)["sim_mean"][0]
    plain = 0.0
    for s in sim:
        plain += float(s)
    assert got == mc.mean_ref(sim) and got != plain / 5000


@needs_compiler
def test_summary_without_retention_times_and_with_foreign_labels(lib):
    labels, sim, pmz, _ = mc.summary_case([3, 4], seed=2)
    labels = labels.copy()
    labels[0] = -1
    labels[1] = 7
    got = hb.summary(lib, labels, 2, sim, pmz)
    want = mc.summary_ref(np.where((labels >= 0) & (labels < 2), labels, 2), 2, sim, pmz)
    for k in mc.COLUMNS:
        assert mc.same(got[k], want[k]), k
    assert not got["rt_min"].any() and not got["rt_max"].any()


@needs_compiler
@pytest.mark.parametrize("form", ["medoid", "consensus"])
def test_member_scores_of_the_host_build(lib, form):
    case, tol = mc.solver_pairs_case(n_pairs=40)
    rep, rep_row = mc.medoid_form(case) if form == "medoid" else mc.consensus_rep(case, tol)
    stats = {}
    want = mc.scores_ref(case, rep, rep_row, tol, stats)
    sim, matched, bad = hb.member_scores(lib, case, rep, rep_row, tol)
    assert not bad and mc.same(sim, want[0]) and mc.same(matched, want[1])
    if form == "medoid":
        assert stats["solver_pairs"] >= 40 and 8 <= stats["max_component"] <= 32
        assert sim.min() >= 0.0 and sim.max() <= 1.0


@needs_compiler
def test_member_scores_tiles_empties_and_the_unsupported_pair(lib):
    case, tol = mc.tile_case(65, "interleaved")
    rep, rep_row = mc.medoid_form(case)
    want = mc.scores_ref(case, rep, rep_row, tol)
    sim, matched, bad = hb.member_scores(lib, case, rep, rep_row, tol)
    assert not bad and mc.same(sim, want[0]) and mc.same(matched, want[1])
    assert (np.diff(case["indptr"]) == 0).any()
    case, rep, rep_row, tol = mc.big_rep_case()
    want = mc.scores_ref(case, rep, rep_row, tol)
    sim, matched, bad = hb.member_scores(lib, case, rep, rep_row, tol)
    assert not bad and mc.same(sim, want[0]) and mc.same(matched, want[1])
    assert not sim[case["labels"] == 2].any() and not matched[case["labels"] == 2].any()
    case, tol = mc.unsupported_case()
    assert hb.member_scores(lib, case, *mc.medoid_form(case), tol)[2]


# ---- summary_io ------------------------------------------------------------------------------------------------------------------
def _blocks():
    b0 = dict(charge="2", cluster=np.array([0, 1], np.int64), labels=np.array([1, 0, 1], np.int64),
              filename=np.array(["a.mgf", "a.mgf", 'dir,x/b "q".mgf']), identifier=np.array(["scan=1", 'id,with "quotes"', "s3"]),
              medoids=np.array([1, 2], np.int64), similarity=np.array([0.5, 1.0, 0.1], np.float32), matched=np.array([3, 7, 1], np.int32),
              size=np.array([1, 2], np.int32), sim_min=np.array([1.0, 0.1], np.float32), worst_row=np.array([1, 2], np.int32),
              sim_mean=np.array([1.0, (float(np.float32(0.5)) + float(np.float32(0.1))) / 2]), pmz_min=np.array([500.25, 600.1], np.float32),
              pmz_max=np.array([500.25, 600.2], np.float32), rt_min=np.array([10.0, 1.5], np.float32),
              rt_max=np.array([10.0, 2.5], np.float32))
    b1 = dict(charge="None", cluster=np.array([2], np.int64), labels=np.array([2], np.int64), filename=np.array(["c.mgf"]),
              identifier=np.array(["only"]), medoids=np.array([0], np.int64), similarity=np.array([1.0000001], np.float32),
              matched=np.array([5], np.int32), size=np.array([1], np.int32), sim_min=np.array([1.0], np.float32),
              worst_row=np.array([0], np.int32), sim_mean=np.array([1.0]), pmz_min=np.array([433.3333], np.float32),
              pmz_max=np.array([433.3333], np.float32), rt_min=np.array([-1.0], np.float32), rt_max=np.array([-1.0], np.float32))
    return [b0, b1]


def test_summary_io_bytes():
    from falcon_amd.ms_io import summary_io
    header = ["falcon version x", "eps = 0.100"]
    f = io.StringIO(newline="")
    summary_io.write_clusters(f, header, _blocks())
    assert f.getvalue() == (
        "# falcon version x\n# eps = 0.100\n#\n"
        "cluster,precursor_charge,size,representative,sim_min,sim_mean,worst,pmz_min,pmz_max,rt_min,rt_max\n"
        '0,2,1,"id,with ""quotes""",1.0,1.0,"id,with ""quotes""",500.25,500.25,10.0,10.0\n'
        "1,2,2,s3,0.1,0.30000000074505806,s3,600.1,600.2,1.5,2.5\n"
        "2,None,1,only,1.0,1.0,only,433.3333,433.3333,-1.0,-1.0\n")
    f = io.StringIO(newline="")
    summary_io.write_scores(f, header, _blocks())
    assert f.getvalue() == (
        "# falcon version x\n# eps = 0.100\n#\n"
        "cluster,filename,identifier,similarity,matched_peaks\n"
        '0,a.mgf,"id,with ""quotes""",1.0,7\n'
        "1,a.mgf,scan=1,0.5,3\n"
        '1,"dir,x/b ""q"".mgf",s3,0.1,1\n'
        "2,c.mgf,only,1.0000001,5\n")


def test_summary_io_writes_both_files(tmp_path):
    from falcon_amd.ms_io import summary_io
    out = str(tmp_path / "run")
    summary_io.write(out, ["h"], _blocks())
    assert open(out + ".clusters.csv", newline="").read().count("\n") == 2 + 1 + 3      # `# h`, `#`, the columns, the rows
    assert open(out + ".scores.csv", newline="").read().count("\n") == 2 + 1 + 4


# ---- config ----------------------------------------------------------------------------------------------------------------------
def test_cluster_summary_parse_errors(capsys):
    from falcon_amd.config import Config
    c = Config()
    with pytest.raises(SystemExit):
        c.parse("in.mgf out --cluster_summary --assign_to reps.mgf")
    assert "--cluster_summary does not combine with --assign_to" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        c.parse("in.mgf out --cluster_summary --distributed")
    assert "--cluster_summary does not combine with --distributed" in capsys.readouterr().err
    c.parse("in.mgf out --cluster_summary --exact")
    assert c.cluster_summary is True
    c.parse("in.mgf out")
    assert c.cluster_summary is False


def test_cluster_summary_from_an_ini_file(tmp_path):
    from falcon_amd.config import Config
    ini = tmp_path / "falcon.ini"
    ini.write_text("cluster_summary = true\neps = 0.2\n")
    c = Config()
    c.parse(f"-c {ini} in.mgf out")
    assert c.cluster_summary is True and c.eps == 0.2
    ini.write_text("cluster_summary = false\n")
    c.parse(f"-c {ini} in.mgf out")
    assert c.cluster_summary is False
    ini.write_text("cluster_summary = true\ndistributed = true\n")
    with pytest.raises(SystemExit):
        c.parse(f"-c {ini} in.mgf out")


def test_option_line_only_with_the_flag_and_never_in_the_file_header():
    from falcon_amd import falcon
    from falcon_amd.config import config
    config.parse("in.mgf out")
    base = falcon._option_lines()
    assert not any("cluster_summary" in l for l in base) and falcon._option_lines(header=True) == base
    header = falcon._header_lines()
    config.parse("in.mgf out --cluster_summary")
    lines = falcon._option_lines()
    assert lines == base + ["cluster_summary = True"]
    # the files' header is what it is without the flag: the cluster CSV does not change with it
    assert falcon._option_lines(header=True) == base and falcon._header_lines() == header


def test_setup_work_dir_guards_the_summary_files_only_with_the_flag(tmp_path):
    from falcon_amd import falcon
    from falcon_amd.config import config
    out = str(tmp_path / "run")
    for ext in (".clusters.csv", ".scores.csv"):
        open(out + ext, "w").close()
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'}")
    assert falcon._setup_work_dir() == (False, 0)
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} --cluster_summary")
    assert falcon._setup_work_dir() == (False, 1)
    config.parse(f"in.mgf {out} --work_dir {tmp_path / 'w'} --cluster_summary --overwrite")
    assert falcon._setup_work_dir() == (False, 0)
    assert not any((tmp_path / ("run" + ext)).exists() for ext in (".clusters.csv", ".scores.csv"))
