"""Cases of tests/test_searchplan_cpu.py and the rules of `csrc/searchplan.h` stated once more in plain Python, from their
descriptions: which kernel a flat bucket takes, the XCD dealing, the batch cuts at the hand-off buffer's cap, the dense4 item
table and the roofline counters.  No GPU, no library: numpy and lists only.  tests/search_batches_worker.py takes the sizes of
its flat case and the batch count it must see from here."""
import itertools

F16, DENSE4, ONE_WAVE, TINY4, EXACT_SMALL, DENSE = range(6)      # searchplan.h: enum FlatKernel
BIG_CAP = 1 << 44                                                # a cap nothing here reaches: one batch


def ceil_div(a, b):
    return -(-a // b)


def block_floats(nq, nc):
    """a job's sims: one [32, nc rounded up to 32] float block per tile of 32 queries"""
    return ceil_div(nq, 32) * 32 * (ceil_div(nc, 32) * 32)


def flat_order(sizes, n_list):
    """non-empty one-list buckets, largest first, equal sizes in bucket order"""
    return sorted((b for b in range(len(sizes)) if n_list[b] == 1 and sizes[b] > 0), key=lambda b: -sizes[b])


def kernel_of(rule, nb):
    have16, have4, has_f32, d, small_max = rule
    if have16 and (not has_f32 or nb >= 64):
        return F16
    if have4 and nb > small_max:
        return DENSE4
    if have4 and nb > 32:
        return ONE_WAVE
    return EXACT_SMALL if d > 512 else TINY4 if have4 else DENSE


def small_max_of(have4, d, env):
    """FALCON_DENSE1_MAX (0: unset) widens the one-wave kernel's range, never below 32, and only up to 512 columns"""
    return max(32, env) if have4 and d <= 512 else 32


def deal(tiles):
    """jobs dealt round-robin to 8 lists -> (every job's tiles in front of it on its list, the longest list)"""
    lists, at = [0] * 8, []
    for j, t in enumerate(tiles):
        at.append(lists[j % 8])
        lists[j % 8] += t
    return at, max(lists)


def plan_flat(sizes, n_list, rule, cap):
    """-> (jobs [(row0, row0, obase, tile0, nb, nb, xtile0)], batches [(j0, jm, js, jk, j1, tiles, lt16, lt32, lt1, floats)], need)
    Buckets in flat_order; a batch takes buckets while their blocks fit the cap (its first bucket always); inside a batch the
    four kernel classes are runs, each dealt to the 8 lists on its own -- the f16 class in 128-row tiles, dense4 not at all."""
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    order = flat_order(sizes, n_list)
    groups, cur, used = [], [], 0
    for b in order:
        f = block_floats(sizes[b], sizes[b])
        if cur and used + f > cap:
            groups.append(cur)
            cur, used = [], 0
        cur.append(b)
        used += f
    if cur:
        groups.append(cur)
    jobs, batches, need = [], [], 0
    for g in groups:
        j0 = len(jobs)
        cls = [kernel_of(rule, sizes[b]) for b in g]
        run = {c: [i for i, k in enumerate(cls) if (k if k < TINY4 else TINY4) == c] for c in (F16, DENSE4, ONE_WAVE, TINY4)}
        xt, longest = {}, {}
        for c, per in ((F16, 128), (ONE_WAVE, 32), (TINY4, 32)):
            at, longest[c] = deal([ceil_div(sizes[g[i]], per) for i in run[c]])
            xt.update(zip(run[c], at))
        obase = tile0 = 0
        for i, b in enumerate(g):
            jobs.append((off[b], off[b], obase, tile0, sizes[b], sizes[b], xt.get(i, 0)))
            obase += block_floats(sizes[b], sizes[b])
            tile0 += ceil_div(sizes[b], 32)
        jm = j0 + len(run[F16])
        js = jm + len(run[DENSE4])
        jk = js + len(run[ONE_WAVE])
        batches.append((j0, jm, js, jk, j0 + len(g), tile0, longest[F16], longest[TINY4], longest[ONE_WAVE], obase))
        need = max(need, obase)
    return jobs, batches, need


def flat_counters(jobs, batches, have4):
    """(pairs, inner products on the matrix cores: 1,024 per 32 x 32 block on or above the diagonal, the same two of the
    one-block buckets where the shared-stream kernels exist: one block each)"""
    pairs = sum(j[4] * j[5] for j in jobs)
    mfma = sum(1024 * (ceil_div(j[5], 32) * (ceil_div(j[5], 32) + 1) // 2) for j in jobs)
    one = [j for b in batches for j in jobs[b[3]:b[4]]] if have4 else []
    return pairs, mfma, sum(j[4] * j[5] for j in one), 1024 * len(one)


def plan_fused(sizes, n_list, k_ann):
    """-> (jobs32, jobs128, longest 32-row list, longest 128-row list, pairs): every flat bucket in 32-row tiles, those with
    more than k_ann rows in 128-row tiles as well, each table dealt on its own"""
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    order = flat_order(sizes, n_list)
    big = [b for b in order if sizes[b] > k_ann]
    at32, l32 = deal([ceil_div(sizes[b], 32) for b in order])
    at128, l128 = deal([ceil_div(sizes[b], 128) for b in big])
    return ([(off[b], off[b], 0, 0, sizes[b], sizes[b], x) for b, x in zip(order, at32)],
            [(off[b], off[b], 0, 0, sizes[b], sizes[b], x) for b, x in zip(big, at128)], l32, l128, sum(sizes[b] ** 2 for b in order))


def plan_coarse(sizes, n_list):
    """indexed buckets in bucket order: rows x the bucket's lists -> (jobs, tiles, floats, the most lists of a bucket)"""
    off, base = [0], [0]
    for s, nl in zip(sizes, n_list):
        off.append(off[-1] + s)
        base.append(base[-1] + nl)
    jobs, tiles, floats = [], 0, 0
    for b, (s, nl) in enumerate(zip(sizes, n_list)):
        if s > 0 and nl != 1:
            jobs.append((off[b], base[b], floats, tiles, s, nl, 0))
            tiles += ceil_div(s, 32)
            floats += block_floats(s, nl)
    return jobs, tiles, floats, max([j[5] for j in jobs], default=0)


def tile_cuts(jobs, cap):
    """tile by tile: a tile that does not fit behind the batch's tiles opens the next batch -> (cuts, need)"""
    cuts, used, need, t = [0], 0, 0, 0
    for j in jobs:
        per = block_floats(32, j[5])
        for _ in range(ceil_div(j[4], 32)):
            if used > 0 and used + per > cap:
                cuts.append(t)
                used = 0
            used += per
            need = max(need, used)
            t += 1
    if cuts[-1] != t:
        cuts.append(t)
    return cuts, need


def bucket_cuts(jobs, qoff, cap):
    """whole buckets: a bucket that takes the batch's span of qoff over the cap opens the next batch -> (batches, need)"""
    out, j0 = [], 0
    span = lambda a, b: qoff[jobs[b][3] + ceil_div(jobs[b][4], 32)] - qoff[jobs[a][3]]
    for j in range(len(jobs)):
        if j > j0 and span(j0, j) > cap:
            out.append((j0, j))
            j0 = j
    out.append((j0, len(jobs)))
    return out, max([span(a, b - 1) for a, b in out if b > a], default=0)


def sorted_tiles32(jobs):
    """the indexed buckets, largest first (stable), as 32-row tiles over their own rows, dealt to the 8 lists"""
    order = sorted(range(len(jobs)), key=lambda i: -jobs[i][4])
    at, longest = deal([ceil_div(jobs[i][4], 32) for i in order])
    return [(jobs[i][0], jobs[i][1], 0, 0, jobs[i][4], jobs[i][4], x) for i, x in zip(order, at)], longest


def dense4_items(nq):
    """-> the table: offsets[0..8] (in items) in a 16-word header, then (job, group) pairs list by list"""
    head, items = [0], []
    for x in range(8):
        for j in range(x, len(nq), 8):
            items += [(j, g) for g in range(ceil_div(nq[j], 128))]
        head.append(len(items))
    return head + [0] * 7 + [w for it in items for w in it]


# ---- cases ----------------------------------------------------------------------------------------------------------------
# rules: (have16, have4, has_f32, d, small_max).  have4 needs float32 rows; an index without any rows is rejected before the plan
RULES = [(h16, h4, f32, d, sm) for (h16, h4, f32), d, sm in
         itertools.product([(1, 1, 1), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 0, 1)], (400, 512, 800), (32, 100))]
EDGE_SIZES = [0, 1, 32, 33, 63, 64, 127, 128, 129, 65535]
# (sizes, n_list): the edge sizes as flat buckets beside indexed and empty ones, with ties (64, 33, 32, 1 twice)
MIXED = ([64, 0, 1, 32, 500, 33, 63, 64, 0, 127, 128, 129, 65535, 33, 700, 32, 1, 101, 100],
         [1, 1, 1, 1, 16, 1, 1, 1, 4, 1, 1, 1, 1, 1, 8, 1, 1, 1, 1])


def per_class(n):
    """n buckets for each of the four classes of rule (0, 1, 1, 400, 100) -- of the f16 class under (1, 1, 1, 400, 100) -- in
    shuffled bucket order"""
    sizes = [140 + 37 * i for i in range(n)] + [33 + (5 * i) % 60 for i in range(n)] + [1 + (3 * i) % 32 for i in range(n)]
    return sizes[1::2] + sizes[0::2]


DEAL_COUNTS = (1, 7, 8, 9, 17)
CAP_1000 = 4194304                                               # FALCON_SIMS_MB=16; a 1,000-row bucket is 1,048,576 floats
# (name, sizes, rule, cap, expected bucket count of every batch)
FLAT_CUTS = [
    ("nine of 1000: 4 + 4 + 1, an exact fit does not cut", [1000] * 9, (0, 1, 1, 64, 32), CAP_1000, [4, 4, 1]),
    ("one bucket over the cap", [3000], (0, 1, 1, 64, 32), CAP_1000, [1]),
    ("one bucket over the cap between others", [3000, 3000, 1000, 20], (0, 1, 1, 64, 32), CAP_1000, [1, 1, 2]),
    ("cut between the f16 prefix and the dense4 part", [40, 1000, 20, 1000, 40, 1000, 20, 40, 1000], (1, 1, 1, 400, 32), CAP_1000,
     [4, 5]),
    ("cut inside the one-wave part", [1000] * 3 + [90] * 120, (0, 1, 1, 400, 100), CAP_1000, None),
]
# the flat case of tests/search_batches_worker.py (low_dim 64, float32 rows only, FALCON_SIMS_MB=16)
GPU_FLAT_SIZES = [1000] * 9 + [20] * 3 + [300] * 2
GPU_FLAT_RULE = (0, 1, 1, 64, 32)
GPU_FLAT_BATCHES = 3

# indexed buckets (rows, lists) with differing list counts; the cap of the tile cuts is 3 tiles of the widest
COARSE = ([100, 700, 0, 33, 50, 1500, 64], [40, 16, 8, 100, 1, 33, 600])
ITEM_CASES = [[], [1], [128], [129], [1, 128, 129, 300, 5, 1000, 64, 257, 640], list(range(1, 40, 3)) + [4000]]
