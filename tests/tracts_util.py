"""IBD tracts in numpy for the tract tests: a run-length encoding of an in-state matrix with
breaks at chromosome starts, and a restatement of scripts/convert_ibd.pl --ibd_pos
(convert_ibd.pl:99-130) applied to an .ibd file's path lines."""
import gzip
import re

import numpy as np


def rle_tracts(state, chrom_start, marg=None, min_sites=1):
    """Maximal runs of True in every row of state [I][S] that no chromosome start (chrom_start
    [S], site 0 counts as one) cuts.  Returns a list of (ind, first_site, n_sites, post_sum)
    (post_sum: the sum of marg [I][S] over the run, 0.0 without marg), ordered by
    (ind, first_site)."""
    state = np.asarray(state).astype(bool)
    I, S = state.shape
    cs = np.asarray(chrom_start, dtype=bool).copy()
    cs[0] = True
    nxt_cs = np.r_[cs[1:], True]
    out = []
    for i in range(I):
        x = state[i]
        prev = np.r_[False, x[:-1]]
        nxt = np.r_[x[1:], False]
        starts = np.flatnonzero(x & (~prev | cs))
        ends = np.flatnonzero(x & (~nxt | nxt_cs))
        assert len(starts) == len(ends)
        for a, b in zip(starts, ends):
            n = int(b - a + 1)
            if n >= min_sites:
                ps = float(marg[i, a:b + 1].sum()) if marg is not None else 0.0
                out.append((i, int(a), n, ps))
    return out


def _read_text(path):
    op = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    with op(path, "rt") as fh:
        return fh.read()


def convert_ibd(ibd_path, pos_path, ind_names):
    """What `convert_ibd.pl --ibd_pos IBD --pos POS --ind NAMES` prints, restated line by line
    from the Perl (convert_ibd.pl:76-130)."""
    sites = []
    for line in _read_text(pos_path).split("\n")[:-1]:
        f = re.split(r"[\t ]", line)
        sites.append((f[0], f[1]))
    last = len(sites) - 1
    out = []
    cur = -1
    for line in _read_text(ibd_path).split("\n")[:-1]:
        if line.startswith("//"):
            continue
        cur += 1
        if cur >= len(ind_names) or ind_names[cur] in ("", "0"):   # next unless ($inds[$curr_ind])
            continue
        s = line.find("1")
        while s != -1:
            chrom = sites[s][0]
            start = int(sites[s][1]) - 1
            while s <= last:
                nxt = line[s + 1:s + 2]
                # substr(...) == 0: Perl's numeric value of the next character
                if s == last or sites[s + 1][0] != chrom or not (nxt.isdigit() and int(nxt) != 0):
                    end = sites[s][1]
                    out.append(f"{chrom}\t{start}\t{end}\t{ind_names[cur]}\t{int(end) - start}\n")
                    s += 1
                    break
                s += 1
            s = line.find("1", s)
    return "".join(out)
