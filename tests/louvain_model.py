"""The synchronous integer Louvain of include/mgpileup.h (mgp_louvain) in plain Python:
integers for every sum, floats for the two products and the difference of a gain, dicts for the
adjacency. Written from the definition, not from the device code; the device must equal it in
every output, bit for bit.

louvain(n, i, j, wq, gamma=1.0, max_levels=32, max_passes=64) -> Model
  i, j, wq: the undirected edges i < j, unique, with integer weights 1..2^20 (units of 2^-20).
"""

from __future__ import annotations

from dataclasses import dataclass, field


@dataclass
class Model:
    labels: list            # per vertex, 0.. by descending community size, ties by smallest member
    n_communities: int
    modularity: float       # Q = S / double(M2) / double(M2)
    m2: int
    internal: int           # I
    b: int                  # B = sum of tot_c^2 (hi = b >> 64, lo = b & (2^64 - 1))
    levels: list = field(default_factory=list)  # (n_vertices, n_communities, passes, accepted)


def score(m2: int, internal: int, b: int, gamma: float) -> float:
    """S = double(M2) * double(I) - gamma * double(B): two products and one difference, each rounded
    on its own; float(int) is the correctly rounded conversion."""
    return float(m2) * float(internal) - gamma * float(b)


def number_labels(raw) -> list:
    """Communities numbered from 0 by descending size, ties by smallest member."""
    members: dict = {}
    for v, c in enumerate(raw):
        members.setdefault(c, []).append(v)
    order = sorted(members.values(), key=lambda m: (-len(m), m[0]))
    out = [0] * len(raw)
    for k, m in enumerate(order):
        for v in m:
            out[v] = k
    return out


def _internal_and_b(adj, self_w, c, tot):
    internal = 0
    for v, row in enumerate(adj):
        internal += self_w[v]
        for u, w in row.items():
            if c[u] == c[v]:
                internal += w
    return internal, sum(t * t for t in tot)


def louvain(n, i, j, wq, gamma: float = 1.0, max_levels: int = 32, max_passes: int = 64) -> Model:
    n, gamma = int(n), float(gamma)
    edges = [(int(a), int(b), int(w)) for a, b, w in zip(i, j, wq)]
    m2 = 2 * sum(w for _, _, w in edges)
    if not edges:  # nothing is launched: every vertex its own community, Q = 0
        return Model(list(range(n)), n, 0.0, 0, 0, 0, [])
    adj = [dict() for _ in range(n)]
    for a, b, w in edges:
        adj[a][b] = w
        adj[b][a] = w
    d = [sum(row.values()) for row in adj]
    self_w = [0] * n
    member = list(range(n))  # the level's vertex of each input vertex
    fm2 = float(m2)
    levels = []
    while True:
        nl = len(adj)
        c = list(range(nl))
        tot = list(d)
        best_i, best_b = _internal_and_b(adj, self_w, c, tot)
        best = score(m2, best_i, best_b, gamma)
        passes = accepted = undone = 0
        while passes < max_passes and undone < 2:
            new = list(c)
            for v in range(nl):
                if not adj[v]:
                    continue
                a = c[v]
                k: dict = {}
                for u, w in adj[v].items():
                    k[c[u]] = k.get(c[u], 0) + w
                g1 = gamma * float(d[v])
                stay = float(k.get(a, 0)) * fm2 - g1 * float(tot[a] - d[v])
                to, to_go = None, 0.0
                for b in sorted(k):  # ascending: a tie keeps the smallest b
                    if b == a or (b > a if passes % 2 == 0 else b < a):
                        continue
                    go = float(k[b]) * fm2 - g1 * float(tot[b])
                    if to is None or go > to_go:
                        to, to_go = b, go
                if to is not None and to_go > stay:
                    new[v] = to
            moved = sum(1 for x, y in zip(c, new) if x != y)
            ntot = [0] * nl
            for v in range(nl):
                ntot[new[v]] += d[v]
            ni, nb = _internal_and_b(adj, self_w, new, ntot)
            s = score(m2, ni, nb, gamma)
            passes += 1
            if moved > 0 and s > best:
                c, tot, best, best_i, best_b = new, ntot, s, ni, nb
                accepted += 1
                undone = 0
            else:
                undone += 1
        # the non-empty communities in ascending label order are the next level's vertices
        ren = {lab: k for k, lab in enumerate(sorted(set(c)))}
        n2 = len(ren)
        levels.append((nl, n2, passes, accepted))
        member = [ren[c[m]] for m in member]
        if n2 == nl or n2 == 1 or len(levels) >= max_levels:
            break
        adj2 = [dict() for _ in range(n2)]
        d2, self2 = [0] * n2, [0] * n2
        for v in range(nl):
            cv = ren[c[v]]
            d2[cv] += d[v]
            self2[cv] += self_w[v]
            for u, w in adj[v].items():
                cu = ren[c[u]]
                if cu == cv:
                    self2[cv] += w
                else:
                    adj2[cv][cu] = adj2[cv].get(cu, 0) + w
        adj, d, self_w = adj2, d2, self2
    q = score(m2, best_i, best_b, gamma) / fm2 / fm2
    labels = number_labels(member)
    return Model(labels, max(labels) + 1 if labels else 0, q, m2, best_i, best_b, levels)
