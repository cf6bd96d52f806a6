"""The pairwise sharing matrices of include/nghmm.h (nghmm_ibd_sharing) restated in numpy for the
sharing tests: from a path [I][S] and a posterior matrix [I][S] over the sites [begin, end).  Counts
are exact integer arithmetic (int64 matrix products of 0/1 values); post_prod is a float64 matrix
product.  Also the text of the command line's PREFIX.ibd.sharing and its parser."""
import numpy as np

HEADER = "ind1\tind2\tvit_both\tpost_both\tpost_prod\n"


def sharing(path, marg, threshold=0.5, begin=0, end=None):
    """(vit_both, post_both, post_prod), each [I][I], over the sites [begin, end)."""
    path = np.asarray(path)
    marg = np.asarray(marg, dtype=np.float64)
    end = path.shape[1] if end is None else end
    assert 0 <= begin < end <= path.shape[1]
    v = (path[:, begin:end] == 1).astype(np.int64)
    q = (marg[:, begin:end] >= threshold).astype(np.int64)
    m = marg[:, begin:end]
    return (v @ v.T).astype(np.uint64), (q @ q.T).astype(np.uint64), m @ m.T


def triple_loop(path, marg, threshold, begin, end):
    """The same definitions as one literal loop per pair and site (small cases only)."""
    I = len(path)
    vit = np.zeros((I, I), dtype=np.uint64)
    both = np.zeros((I, I), dtype=np.uint64)
    prod = np.zeros((I, I), dtype=np.float64)
    for i in range(I):
        for j in range(I):
            v = b = 0
            x = 0.0
            for s in range(begin, end):
                if path[i][s] == 1 and path[j][s] == 1:
                    v += 1
                if marg[i][s] >= threshold and marg[j][s] >= threshold:
                    b += 1
                x += float(marg[i][s]) * float(marg[j][s])
            vit[i, j], both[i, j], prod[i, j] = v, b, x
    return vit, both, prod


def sharing_text(vit, both, prod, ids):
    """PREFIX.ibd.sharing: the header, then one line per pair i <= j in (i, j) order."""
    out = [HEADER]
    for i in range(len(ids)):
        for j in range(i, len(ids)):
            out.append("%s\t%s\t%d\t%d\t%.10g\n" % (ids[i], ids[j], int(vit[i, j]), int(both[i, j]),
                                                    float(prod[i, j])))
    return "".join(out)


def parse_sharing(text, n_ind):
    """(ids [I], vit_both, post_both, post_prod) of a PREFIX.ibd.sharing file's text: the full
    symmetric matrices."""
    lines = text.split("\n")
    assert lines[0] + "\n" == HEADER and lines[-1] == "" and len(lines) == 2 + n_ind * (n_ind + 1) // 2
    vit = np.zeros((n_ind, n_ind), dtype=np.uint64)
    both = np.zeros((n_ind, n_ind), dtype=np.uint64)
    prod = np.zeros((n_ind, n_ind), dtype=np.float64)
    ids = [None] * n_ind
    k = 1
    for i in range(n_ind):
        for j in range(i, n_ind):
            f = lines[k].split("\t")
            k += 1
            assert len(f) == 5
            for who, name in ((i, f[0]), (j, f[1])):
                assert ids[who] in (None, name)
                ids[who] = name
            vit[i, j] = vit[j, i] = int(f[2])
            both[i, j] = both[j, i] = int(f[3])
            prod[i, j] = prod[j, i] = float(f[4])
    return ids, vit, both, prod
