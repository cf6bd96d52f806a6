"""The region and site summaries of include/nghmm.h (nghmm_ibd_summary) restated in numpy for the
summary tests: from a path [I][S], a posterior matrix [I][S], the distances [S] and regions [R][2].
Counts are exact integer arithmetic; sums are np.add.reduce.  Also the text of the command line's
PREFIX.ibd.regions / PREFIX.ibd.sites, and a reader of an .ibd file's path and posterior lines."""
import gzip
import re

import numpy as np

REGION_DTYPE = np.dtype([("vit_sites", np.uint64), ("post_sites", np.uint64),
                         ("post_sum", np.float64), ("vit_mb", np.float64)])
SITE_DTYPE = np.dtype([("vit_count", np.uint32), ("post_count", np.uint32), ("post_sum", np.float64)])


def mb_terms(path_row, pos_dist, a, b):
    """The distances that make up vit_mb of one individual in the region [a, b): d_s of the sites
    a < s < b with path[s - 1] == path[s] == 1 and d_s finite."""
    s = np.arange(a + 1, b)
    sel = (path_row[s - 1] != 0) & (path_row[s] != 0) & np.isfinite(pos_dist[s])
    return pos_dist[s[sel]]


def summarize(path, marg, pos_dist, regions, threshold=0.5, viterbi=True, posterior=True):
    """(region_stats [I][R], site_stats [S], n_terms): the records, and per region record the
    number of terms of vit_mb (for the tests' bounds).  The fields of a source that is switched
    off are 0."""
    path = np.asarray(path)
    marg = np.asarray(marg, dtype=np.float64)
    d = np.asarray(pos_dist, dtype=np.float64)
    I, S = path.shape
    regions = np.asarray(regions, dtype=np.int64).reshape(-1, 2)
    R = len(regions)
    reg = np.zeros((I, R), dtype=REGION_DTYPE)
    n_mb = np.zeros((I, R), dtype=np.int64)
    sites = np.zeros(S, dtype=SITE_DTYPE)
    vit = path != 0
    hit = marg >= threshold
    for r, (a, b) in enumerate(regions):
        assert 0 <= a < b <= S
        for i in range(I):
            if viterbi:
                reg["vit_sites"][i, r] = int(np.count_nonzero(vit[i, a:b]))
                t = mb_terms(path[i], d, a, b)
                n_mb[i, r] = len(t)
                reg["vit_mb"][i, r] = np.add.reduce(t) if len(t) else 0.0
            if posterior:
                reg["post_sites"][i, r] = int(np.count_nonzero(hit[i, a:b]))
                reg["post_sum"][i, r] = np.add.reduce(marg[i, a:b])
    if viterbi:
        sites["vit_count"] = np.count_nonzero(vit, axis=0)
    if posterior:
        sites["post_count"] = np.count_nonzero(hit, axis=0)
        sites["post_sum"] = np.add.reduce(marg, axis=0)
    return reg, sites, n_mb


def triple_loop(path, marg, pos_dist, regions, threshold):
    """The same definitions as one literal loop per record (small cases only)."""
    I, S = path.shape
    reg = np.zeros((I, len(regions)), dtype=REGION_DTYPE)
    sites = np.zeros(S, dtype=SITE_DTYPE)
    for i in range(I):
        for r, (a, b) in enumerate(regions):
            vs = ps = 0
            psum = mb = 0.0
            for s in range(a, b):
                if path[i][s] == 1:
                    vs += 1
                if marg[i][s] >= threshold:
                    ps += 1
                psum += float(marg[i][s])
                if s > a and path[i][s - 1] == 1 and path[i][s] == 1 and np.isfinite(pos_dist[s]):
                    mb += float(pos_dist[s])
            reg[i, r] = (vs, ps, psum, mb)
    for s in range(S):
        vc = pc = 0
        psum = 0.0
        for i in range(I):
            vc += int(path[i][s] == 1)
            pc += int(marg[i][s] >= threshold)
            psum += float(marg[i][s])
        sites[s] = (vc, pc, psum)
    return reg, sites


def _read_text(path):
    op = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    with op(path, "rt") as fh:
        return fh.read()


def read_pos(pos_path):
    """(chromosome names [S], positions [S], distances in Mb [S] with inf at chromosome starts)
    of a --pos file, as the host reads it."""
    names, pos = [], []
    for line in _read_text(pos_path).split("\n")[:-1]:
        f = re.split(r"[\t ]", line)
        names.append(f[0])
        pos.append(int(f[1]))
    d = np.full(len(pos), np.inf)
    for s in range(1, len(pos)):
        if names[s] == names[s - 1]:
            d[s] = (float(pos[s]) - float(pos[s - 1])) / 1e6
    return names, pos, d


def read_ibd(ibd_path, n_ind):
    """(path [I][S] uint8, posteriors [I][S] as printed with "%f") of an .ibd file."""
    lines = _read_text(ibd_path).split("\n")[:-1]
    assert lines[0].startswith("//") and len(lines) == 1 + 2 * n_ind
    path = np.array([[int(c) for c in l] for l in lines[1:1 + n_ind]], dtype=np.uint8)
    marg = np.array([[float(v) for v in l.split("\t")] for l in lines[1 + n_ind:]])
    return path, marg


def chrom_regions(names, window=0):
    """The command line's regions: the runs of one chromosome name, or windows of `window` sites
    that restart at every such run."""
    S = len(names)
    first = [s for s in range(S) if s == 0 or names[s] != names[s - 1]]
    out = []
    for a, b in zip(first, first[1:] + [S]):
        w = window or b - a
        out += [(lo, min(lo + w, b)) for lo in range(a, b, w)]
    return np.array(out, dtype=np.int64)


REGIONS_HEADER = "ind\tchr\tfirst_pos\tlast_pos\tn_sites\tvit_sites\tvit_share\tpost_sites\tpost_mean\tvit_mb\n"
SITES_HEADER = "chr\tpos\tvit_count\tpost_count\tpost_mean\n"


def regions_text(reg, regions, names, pos, ids):
    out = [REGIONS_HEADER]
    for i in range(reg.shape[0]):
        for r, (a, b) in enumerate(regions):
            t, n = reg[i, r], int(b - a)
            out.append("%s\t%s\t%d\t%d\t%d\t%d\t%.10g\t%d\t%.10g\t%.10g\n" % (
                ids[i], names[a], pos[a], pos[b - 1], n, int(t["vit_sites"]), int(t["vit_sites"]) / n,
                int(t["post_sites"]), float(t["post_sum"]) / n, float(t["vit_mb"])))
    return "".join(out)


def sites_text(sites, names, pos, n_ind):
    out = [SITES_HEADER]
    for s in range(len(sites)):
        t = sites[s]
        out.append("%s\t%d\t%d\t%d\t%.10g\n" % (names[s], pos[s], int(t["vit_count"]),
                                                  int(t["post_count"]), float(t["post_sum"]) / n_ind))
    return "".join(out)
