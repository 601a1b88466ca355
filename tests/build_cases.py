"""Cases of tests/test_buildplan_cpu.py and the rules of `csrc/buildplan.h` stated once more in plain Python, from their
descriptions: the list table of a bucket table, which assignment kernel a bucket's k-means passes take, the job tables of those
kernels, and the small rules of the list sort, the sparsify launch and the coarse keys.  No GPU, no library: lists only.
tests/test_gpu_search.py takes the bucket table of its every-class build from here."""

SEG, GROUP, MAX_LISTS, MERGE_LISTS, SORT_MAX_LISTS = 2048, 128, 512, 2048, 2048      # buildplan.h: kAssign*, kBucketSortMaxLists
MAX_N_LIST = 131072                                                                # include/falcon_hip.h: FAL_MAX_N_LIST
INT32_MAX = 2 ** 31 - 1
SINGLE, MERGE, WAVE, WIDE, DENSE = "single", "merge", "wave", "wide", "dense"


def ceil_div(a, b):
    return -(-a // b)


def offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


def first_bad_bucket(off, n_list, max_n_list=MAX_N_LIST):
    """-1, or the first bucket with a negative size, a list count outside [1, max_n_list] or above its (non-zero) rows, or more
    than INT32_MAX rows"""
    for b, nl in enumerate(n_list):
        nb = off[b + 1] - off[b]
        if nb < 0 or nl < 1 or nl > max_n_list or (nb > 0 and nl > nb) or nb > INT32_MAX:
            return b
    return -1


def list_table(off, n_list):
    """-> (list_base [buckets + 1], indexed buckets [(row0, list0, rows, n_list, wave0)], total lists, waves): every bucket's
    lists follow the previous bucket's; an indexed bucket (more than one list) takes one wave per list"""
    base = offsets(n_list)
    bk, waves = [], 0
    for b, nl in enumerate(n_list):
        if nl > 1:
            bk.append((off[b], base[b], off[b + 1] - off[b], nl, waves))
            waves += nl
    return base, bk, base[-1], waves


def class_of(n_list, use16):
    """the kernel class of an indexed bucket's assignment passes"""
    if use16 and n_list <= GROUP:
        return SINGLE
    if use16 and n_list <= MERGE_LISTS:
        return MERGE
    return WAVE if n_list <= 64 else WIDE if n_list <= MAX_LISTS else DENSE


def seg_rows(work_rows, num_cus, per_cu):
    """rows per job: at least `per_cu` workgroups per CU, a multiple of 32 between 256 and SEG"""
    return min(SEG, max(256, 32 * ceil_div(work_rows, num_cus * per_cu * 32)))


def segments(row0, rows, seg):
    return [(row0 + s, min(seg, rows - s)) for s in range(0, rows, seg)]


def groups(n_list, width):
    return [(t, min(width, n_list - t)) for t in range(0, n_list, width)]


def plan_assign(bk, num_cus, use16):
    """-> dict: `wide` = the n_wide 4-wave jobs then the n_wave one-wave jobs, `half` = the n_single single-group, n_merge merge and
    n_group group jobs (jobs: (row0, cent0, nrows, ncent, id_base, part0)), `dense` = (q_row0, c_row0, 0, tile0, nq, nc, 0), and
    the scalars.  seg / wseg count the work of every bucket with 65..512 / up to 64 lists, whichever class it takes in the end."""
    seg = seg_rows(sum(n * ceil_div(nl, GROUP) for _, _, n, nl, _ in bk if 64 < nl <= MAX_LISTS), num_cus, 4)
    wseg = seg_rows(sum(n * ceil_div(nl, 32) for _, _, n, nl, _ in bk if nl <= 64), num_cus, 16)
    single, merge, group, wave, wide, dense = [], [], [], [], [], []
    merge_rows = dtiles = merge_max = 0
    for row0, list0, n, nl, _ in bk:
        cls = class_of(nl, use16)
        if cls == SINGLE:
            single += [(r, list0, nr, nl, 0, 0) for r, nr in segments(row0, n, SEG)]
        elif cls == MERGE:
            merge_max = max(merge_max, nl)
            for r, nr in segments(row0, n, SEG):               # part0: the rows of every merge segment in front of this one
                merge.append((r, list0, nr, nl, 0, merge_rows))
                group += [(r, list0 + t, nr, nc, t, merge_rows) for t, nc in groups(nl, GROUP)]
                merge_rows += nr
        elif cls == WAVE:
            wave += [(r, list0 + t, nr, nc, t, 0) for r, nr in segments(row0, n, wseg) for t, nc in groups(nl, 32)]
        elif cls == WIDE:
            wide += [(r, list0 + t, nr, nc, t, 0) for r, nr in segments(row0, n, seg) for t, nc in groups(nl, GROUP)]
        else:
            dense.append((row0, list0, 0, dtiles, n, nl, 0))
            dtiles += ceil_div(n, 32)
    return dict(wide=wide + wave, n_wide=len(wide), n_wave=len(wave), half=single + merge + group, n_single=len(single),
                n_merge=len(merge), n_group=len(group), dense=dense, dtiles=dtiles, merge_rows=merge_rows, merge_max_lists=merge_max,
                max_n_list=max([nl for _, _, _, nl, _ in bk], default=0), seg=seg, wseg=wseg)


def end_bit(total):
    """key bits of the list sort: enough for ids below `total`, between 1 and 32"""
    return min(32, max(1, (total - 1).bit_length())) if total > 1 else 1


def sparsify_segments(bk):
    return offsets([ceil_div(n, 256) for _, _, n, _, _ in bk])


def ckeys_stride(max_n_list):
    return GROUP * ceil_div(max_n_list, GROUP)


def initial_counts(off, n_list):
    base = offsets(n_list)
    cnt = [0] * (base[-1] + 1)
    for b, nl in enumerate(n_list):
        if nl == 1:
            cnt[base[b]] = off[b + 1] - off[b]
    return cnt


def flat_list_off(off):
    """every bucket one list: list g ends where bucket g ends"""
    return list(off)


# ---- cases -----------------------------------------------------------------------------------------------------------------
EDGE_LISTS = [1, 2, 32, 33, 64, 65, 128, 129, 512, 513, 2048, 2049]
NUM_CUS = [1, 256, 8, 3]                 # 8 and 3 put seg / wseg of the tables below between and at their clamps


def rows_for(n_list, factor=4, least=40):
    return max(least, factor * n_list)


# one bucket per edge list count, about four rows per list; flat buckets (some empty) in between
EDGE_TABLE = ([rows_for(nl) for nl in EDGE_LISTS] + [0, 7], EDGE_LISTS + [1, 1])
# bucket sizes at the segment cuts, for a list count of every class; a bucket with as many rows as lists; an empty indexed bucket
CUT_SIZES = [2048, 2049, 4097]
CUT_LISTS = [2, 64, 65, 129, 513]
SIZE_TABLE = ([s for nl in CUT_LISTS for s in CUT_SIZES] + [33, 129, 0], [nl for nl in CUT_LISTS for _ in CUT_SIZES] + [33, 129, 5])
# two merge buckets in a row (with use16): part0 runs on over both, the group jobs of a segment are adjacent
TWO_MERGE = ([4200, 100, 2100, 3000], [129, 1, 300, 16])
LONG = ([40000, 30000], [64, 200])      # on one CU both segment lengths reach SEG
TABLES = {"edges": EDGE_TABLE, "sizes": SIZE_TABLE, "two merge buckets": TWO_MERGE, "long": LONG,
          "all flat": ([5, 0, 0, 9, 0], [1] * 5), "none": ([], [])}

# (name, sizes or offsets, n_list, first bad bucket); offsets where a size cannot say it
INVALID = [
    ("negative size", dict(off=[0, 10, 5, 20]), [1, 1, 1], 1),
    ("n_list 0", dict(sizes=[10, 10]), [1, 0], 1),
    ("n_list negative", dict(sizes=[10, 10]), [-3, 1], 0),
    ("n_list above the limit", dict(sizes=[MAX_N_LIST + 2]), [MAX_N_LIST + 1], 0),
    ("n_list at the limit is valid", dict(sizes=[MAX_N_LIST]), [MAX_N_LIST], -1),
    ("more lists than rows", dict(sizes=[40, 7, 40]), [2, 8, 2], 1),
    ("as many lists as rows is valid", dict(sizes=[8]), [8], -1),
    ("an empty bucket may have lists", dict(sizes=[0, 4]), [5, 2], -1),
    ("more than INT32_MAX rows", dict(sizes=[5, INT32_MAX + 1]), [1, 1], 1),
    ("INT32_MAX rows is valid", dict(sizes=[INT32_MAX]), [1], -1),
    ("the first of two bad buckets", dict(sizes=[10, 3, 10, 2]), [1, 4, 1, 0], 1),
]

# the GPU test's index: every class side by side (tests/test_gpu_search.py); 4,200 rows on 129 lists = three segments, so the
# merge jobs of the buckets behind it start at part0 > 0.  2,049 lists: the one count the float16 assignment leaves to dense
GPU_LISTS = [1, 2, 64, 65, 128, 129, 512, 513, 2049]
GPU_SIZES = [4200 if nl == 129 else rows_for(nl) for nl in GPU_LISTS]
GPU_CLASSES = {True: {SINGLE: [2, 64, 65, 128], MERGE: [129, 512, 513], DENSE: [2049]},
               False: {WAVE: [2, 64], WIDE: [65, 128, 129, 512], DENSE: [513, 2049]}}
