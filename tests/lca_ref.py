"""The LCA assignment of DESIGN.md section 4 restated in Python, for the tests of mm_lca_core.hpp, mm_em_lca and `classify --lca`:
mass(r, v) = sum of the posteriors of read r's entries whose node lies in the subtree of v, by walking every entry's parents;
lca(r) = the deepest node with mass(r, v) >= tau - 1e-9, the root if there is none."""
import numpy as np

SLACK = 1e-9


def depths(parent):
    d = np.zeros(len(parent), dtype=np.int64)
    for v in range(1, len(parent)):
        d[v] = d[parent[v]] + 1
    return d


def brute_one(parent, depth, nodes, p, tau):
    """one read, straight from the definition: (lca, mass of the lca, {node: mass} of every node with an entry below it)"""
    mass = {}
    for v, x in zip(nodes, p):
        v = int(v)
        while True:
            mass[v] = mass.get(v, 0.0) + float(x)
            if v == 0:
                break
            v = int(parent[v])
    ok = [v for v, m in mass.items() if m >= tau - SLACK]
    best = max(ok, key=lambda v: depth[v]) if ok else 0
    assert sum(1 for v in ok if depth[v] == depth[best]) <= 1, "two qualifying nodes of one depth"
    return best, mass[best], mass


def assign(parent, read_off, node, p, tau, margin=None):
    """all reads at once.  tau: one value or one per read.  Returns (lca [n_reads] int32, -1 without entries; mass [n_reads]; direct [n_nodes];
    near [n_reads] bool: some node mass of the read within `margin` of tau - 1e-9, all False without a margin)."""
    parent = np.asarray(parent, dtype=np.int64)
    read_off = np.asarray(read_off, dtype=np.int64)
    node = np.asarray(node, dtype=np.int64)
    p = np.asarray(p, dtype=np.float64)
    n_nodes, n_reads = len(parent), len(read_off) - 1
    depth = depths(parent)
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (n_reads,))
    rd = np.repeat(np.arange(n_reads, dtype=np.int64), np.diff(read_off))
    keys, vals = [], []
    idx, cur = np.arange(len(node)), node.copy()
    while len(idx):
        keys.append(rd[idx] * n_nodes + cur[idx])
        vals.append(p[idx])
        idx = idx[cur[idx] != 0]
        cur[idx] = parent[cur[idx]]
    lca = np.full(n_reads, -1, dtype=np.int32)
    mass = np.zeros(n_reads, dtype=np.float64)
    near = np.zeros(n_reads, dtype=bool)
    direct = np.zeros(n_nodes, dtype=np.int64)
    if not keys:
        return lca, mass, direct, near
    uniq, inv = np.unique(np.concatenate(keys), return_inverse=True)
    m = np.zeros(len(uniq), dtype=np.float64)
    np.add.at(m, inv, np.concatenate(vals))
    r, v = uniq // n_nodes, uniq % n_nodes
    if margin is not None:
        near[r[np.abs(m - (tau[r] - SLACK)) <= margin]] = True
    root = v == 0                                                  # every read with entries has its root key: the fallback
    lca[r[root]], mass[r[root]] = 0, m[root]
    ok = m >= tau[r] - SLACK
    r, v, m = r[ok], v[ok], m[ok]
    order = np.lexsort((depth[v], r))                              # by read, then depth: the last of a read is its deepest
    r, v, m = r[order], v[order], m[order]
    last = np.append(r[1:] != r[:-1], True) if len(r) else np.zeros(0, dtype=bool)
    lca[r[last]], mass[r[last]] = v[last], m[last]
    np.add.at(direct, lca[lca >= 0], 1)
    return lca, mass, direct, near


def exact_posteriors(rng, n, alpha=None):
    """n multiples of 2^-20, each at least 2^-20, that sum to exactly 1"""
    w = rng.dirichlet(np.full(n, alpha if alpha else rng.choice([0.05, 0.3, 1.0, 5.0])))
    k = rng.multinomial((1 << 20) - n, w) + 1
    return k.astype(np.float64) / float(1 << 20)


def random_tree(rng, n, shape):
    """parent[] with parent[v] < v: 'chain', 'star', 'random' (uniform earlier node) or 'deep' (a recent node: long paths)"""
    parent = np.zeros(n, dtype=np.int32)
    for v in range(1, n):
        if shape == "chain":
            parent[v] = v - 1
        elif shape == "star":
            parent[v] = 0
        elif shape == "deep":
            parent[v] = rng.integers(max(0, v - 3), v)
        else:
            parent[v] = rng.integers(0, v)
    return parent
