"""Synthetic SPD test matrices and geometric partitions, generated from their
definition (no files, no downloads): the 7-point Poisson operator of SURVEY
Appendix A.2 and sub-box partitions of the grid (the stand-in for METIS k-way
on structured problems)."""
import numpy as np


def poisson3d_csr(n):
    """A = T(x)I(x)I + I(x)T(x)I + I(x)I(x)T, T = tridiag(-1, 2, -1); row (i*n+j)*n+k.
    Returns int32 rowptr, int32 colind, float64 val with sorted columns."""
    N = n ** 3
    idx = np.arange(N, dtype=np.int64)
    i, j, k = idx // (n * n), (idx // n) % n, idx % n
    cols = [idx - n * n, idx - n, idx - 1, idx, idx + 1, idx + n, idx + n * n]
    ok = [i > 0, j > 0, k > 0, np.ones(N, bool), k < n - 1, j < n - 1, i < n - 1]
    vals = [-1.0, -1.0, -1.0, 6.0, -1.0, -1.0, -1.0]
    C = np.stack(cols, axis=1)
    M = np.stack(ok, axis=1)
    V = np.broadcast_to(np.array(vals), (N, 7))
    counts = M.sum(axis=1)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(counts)
    return rowptr.astype(np.int32), C[M].astype(np.int32), np.ascontiguousarray(V[M], dtype=np.float64)


def graded_values(rowptr, colind, val, lo, hi):
    """The values of S A S, S = diag(10^g), g = linspace(lo, hi, N): the same pattern, still SPD (a congruence), with
    a coefficient graded over hi - lo decades.  The row scaling of the solver equilibrates it, so a residual norm
    in the scaled space and one in the caller's units weigh the rows differently by up to 10^(hi - lo)."""
    N = len(rowptr) - 1
    sc = 10.0 ** np.linspace(lo, hi, N)
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    return sc[rows] * np.asarray(val, dtype=np.float64) * sc[colind]


def box_partition(n, box):
    """Part id of every node of an n^3 grid cut into boxes of `box` = (bi, bj, bk)
    nodes (the last box of a direction may be smaller).  Parts are numbered
    box-lexicographically, so consecutive parts are neighbours."""
    bi, bj, bk = box
    idx = np.arange(n ** 3, dtype=np.int64)
    i, j, k = idx // (n * n), (idx // n) % n, idx % n
    ni, nj, nk = -(-n // bi), -(-n // bj), -(-n // bk)
    part = ((i // bi) * nj + (j // bj)) * nk + (k // bk)
    return part.astype(np.int32), ni * nj * nk


def q1_elasticity_element(nu=0.25, E=1.0):
    """24 x 24 stiffness of the trilinear (Q1) unit-cube element of isotropic linear
    elasticity, 2x2x2 Gauss quadrature.  Node order (1,0,0)-first counter-clockwise on the
    bottom face, then the top face, dof = 3*node + component: the ordering the reference's
    assembly uses (examples/test_ecg_petsc_ela.c:294-301).  The reference hard-codes its own
    24 x 24 table (reference_q1_element below, the default of elasticity3d_csr); this one is
    derived from the definition, so values differ while the sparsity, block structure and
    SPD-ness are the same."""
    lam = E * nu / ((1 + nu) * (1 - 2 * nu))
    mu = E / (2 * (1 + nu))
    D = np.zeros((6, 6))
    D[:3, :3] = lam
    D[np.arange(3), np.arange(3)] += 2 * mu
    D[np.arange(3, 6), np.arange(3, 6)] = mu
    corners = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], float)
    g = 0.5 + np.array([-1.0, 1.0]) / (2 * np.sqrt(3.0))
    K = np.zeros((24, 24))
    for x in g:
        for y in g:
            for z in g:
                p = np.array([x, y, z])
                f = np.where(corners == 1, p, 1 - p)           # 1-D factors per node and axis
                df = np.where(corners == 1, 1.0, -1.0)
                dN = np.stack([df[:, 0] * f[:, 1] * f[:, 2], f[:, 0] * df[:, 1] * f[:, 2],
                               f[:, 0] * f[:, 1] * df[:, 2]], axis=1)   # (8, 3)
                B = np.zeros((6, 24))
                for a in range(8):
                    dx, dy, dz = dN[a]
                    B[0, 3 * a] = dx
                    B[1, 3 * a + 1] = dy
                    B[2, 3 * a + 2] = dz
                    B[3, 3 * a], B[3, 3 * a + 1] = dy, dx
                    B[4, 3 * a + 1], B[4, 3 * a + 2] = dz, dy
                    B[5, 3 * a], B[5, 3 * a + 2] = dz, dx
                K += B.T @ D @ B / 8.0
    return 0.5 * (K + K.T)


def reference_q1_element():
    """The reference's own 24 x 24 element matrix `elem_3d_elast_v_25`
    (examples/test_ecg_petsc_ela.c:65-211), exact: integer numerators over 1080."""
    from .q1_table import Q1_DENOMINATOR, Q1_NUMERATORS
    return np.array(Q1_NUMERATORS, dtype=np.float64) / float(Q1_DENOMINATOR)


def _dims(nn):
    if np.isscalar(nn):
        return int(nn), int(nn), int(nn)
    nx, ny, nz = (int(v) for v in nn)
    return nx, ny, nz


def elasticity3d_csr(nn, nu=0.25, element="reference"):
    """Q1 3-D elasticity on nn^3 nodes -- or (nx, ny, nz) nodes -- assembled the way
    examples/test_ecg_petsc_ela.c:217-347 does for one process: node id = i + nx*j + nx*ny*k,
    dof = 3*node + c, N = 3 nx ny nz; element coefficient 1 except 1e-5 / 1e5 where the element
    centre lies within 0.05 of one of the eight points (.25|.75)^3 of the unit cube (lines
    275-323, tested in the reference's order); in the k = 0 element layer the bottom-face nodes
    are decoupled and their diagonal scaled by 0.1 (DD2, lines 234-246), which keeps the matrix
    SPD without eliminating rows.  element = "reference": the reference's own element matrix
    (q1_table.py); "derived": the textbook Q1 stiffness for Poisson ratio nu by 2x2x2 Gauss
    quadrature (same sparsity and block structure, different values).  The reference only
    generates cubes; on a box the unit cube is cut into nx-1 x ny-1 x nz-1 elements and the
    (size-independent) element matrix is kept.  Returns int32 rowptr, int32 colind, float64 val."""
    nx, ny, nz = _dims(nn)
    ex, ey, ez = nx - 1, ny - 1, nz - 1
    if element == "reference":
        DD1 = reference_q1_element()
    elif element == "derived":
        DD1 = q1_elasticity_element(nu)
    else:
        raise ValueError("element must be 'reference' or 'derived'")
    DD2 = DD1.copy()
    for a in range(24):
        for b in range(24):
            if a < 12 or b < 12:
                DD2[a, b] = 0.1 * DD1[a, a] if a == b else 0.0
    # element coefficient, indexed [i, j, k]
    cx, cy, cz = ((np.arange(e) + 0.5) / e for e in (ex, ey, ez))
    X, Y, Z = np.meshgrid(cx, cy, cz, indexing="ij")      # element centres
    alpha = np.ones((ex, ey, ez))
    r = 0.05
    order = [((.25, .25, .25), (.25, .25, .75), 1e-5), ((.75, .25, .25), (.75, .25, .75), 1e5),
             ((.25, .75, .25), (.25, .75, .75), 1e-5), ((.75, .75, .25), (.75, .75, .75), 1e5)]
    for c1, c2, val in order:
        for px, py, pz in (c1, c2):
            alpha[np.sqrt((X - px) ** 2 + (Y - py) ** 2 + (Z - pz) ** 2) < r] = val
    corners = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    # node-block accumulation: blocks[i, j, k, offset(di,dj,dk), 3, 3]
    blocks = np.zeros((nx, ny, nz, 27, 3, 3))
    for a, ca in enumerate(corners):
        for b, cb in enumerate(corners):
            off = ((cb[2] - ca[2] + 1) * 3 + (cb[1] - ca[1] + 1)) * 3 + (cb[0] - ca[0] + 1)
            blk1 = DD1[3 * a:3 * a + 3, 3 * b:3 * b + 3]
            blk2 = DD2[3 * a:3 * a + 3, 3 * b:3 * b + 3]
            # element (i,j,k) contributes to node (i+ca0, j+ca1, k+ca2)
            tgt = blocks[ca[0]:ca[0] + ex, ca[1]:ca[1] + ey, ca[2]:ca[2] + ez, off]
            tgt[:, :, 1:] += alpha[:, :, 1:, None, None] * blk1
            tgt[:, :, :1] += alpha[:, :, :1, None, None] * blk2
    # CSR: node rows in id order (k slowest), neighbours in increasing node id
    I, J, K_ = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    node = (I + nx * J + nx * ny * K_)
    offs = [(di, dj, dk) for dk in (-1, 0, 1) for dj in (-1, 0, 1) for di in (-1, 0, 1)]
    exist = np.zeros((nx, ny, nz, 27), bool)
    nbr = np.zeros((nx, ny, nz, 27), np.int64)
    for o, (di, dj, dk) in enumerate(offs):
        ok = ((I + di >= 0) & (I + di < nx) & (J + dj >= 0) & (J + dj < ny) & (K_ + dk >= 0) & (K_ + dk < nz))
        exist[..., o] = ok
        nbr[..., o] = node + di + nx * dj + nx * ny * dk
    perm = np.argsort(node.ravel())                     # row order = node id
    exist = exist.reshape(-1, 27)[perm]
    nbr = nbr.reshape(-1, 27)[perm]
    blocks = blocks.reshape(-1, 27, 3, 3)[perm]
    cnt = exist.sum(axis=1)                             # neighbours per node
    nnodes = nx * ny * nz
    rowptr = np.zeros(3 * nnodes + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.repeat(3 * cnt, 3))
    nb_flat = nbr[exist]                                # (sum cnt,) in node-major, offset-minor order
    bl_flat = blocks[exist]                             # (sum cnt, 3, 3)
    node_of = np.repeat(np.arange(nnodes), cnt)
    first = np.zeros(nnodes + 1, dtype=np.int64)
    first[1:] = np.cumsum(cnt)
    pos_in_row = np.arange(len(nb_flat)) - first[node_of]
    colind = np.empty(rowptr[-1], dtype=np.int32)
    val = np.empty(rowptr[-1], dtype=np.float64)
    for ci in range(3):                                 # row component
        base = rowptr[3 * node_of + ci] + 3 * pos_in_row
        for cj in range(3):
            colind[base + cj] = 3 * nb_flat + cj
            val[base + cj] = bl_flat[:, ci, cj]
    return rowptr.astype(np.int32), colind, val


def box_partition_nodes(nn, box, dofs=3):
    """box_partition for a vector problem with `dofs` unknowns per node (dof = dofs*node + c,
    node id = i + nx*j + nx*ny*k) on nn^3 or (nx, ny, nz) nodes."""
    nx, ny, nz = _dims(nn)
    bi, bj, bk = box
    nid = np.arange(nx * ny * nz, dtype=np.int64)
    i, j, k = nid % nx, (nid // nx) % ny, nid // (nx * ny)
    ni, nj, nk = -(-nx // bi), -(-ny // bj), -(-nz // bk)
    part = ((k // bk) * nj + (j // bj)) * ni + (i // bi)
    return np.repeat(part, dofs).astype(np.int32), ni * nj * nk


def node_graph_csr(nn, stride, seed, far_every=7, nfar=2, excess=1.0):
    """SPD matrix of a graph of nn nodes with three dofs per node (dof = 3*node + c): every row has its nonzeros in
    runs of three consecutive columns and only a few of them, so a host product of 3 nn rows takes a fraction of a
    second.  Links: i -- i+1 and i -- i+stride; every far_every-th node (0, far_every, ...) also gets nfar links to
    nodes drawn with rng.integers(0, nn) (nfar draws of one node per such node, in that order; a self link is
    dropped).  The graph is symmetrised and gets the identity; every link becomes a dense 3 x 3 block of values
    -rng.random() (drawn in CSR order of the 3 nn x 3 nn pattern), the matrix is symmetrised by (A + A^T) / 2 and the
    diagonal is set to (1 + excess) * sum |off-diagonal| of its row: strictly diagonally dominant, the smaller excess
    the worse conditioned.  Returns int32 rowptr, int32 colind, float64 val with sorted columns."""
    import scipy.sparse as sp
    nn, stride = int(nn), int(stride)
    if nn < 2 or not 0 < stride < nn or far_every < 1 or nfar < 0 or excess <= 0.0:
        raise ValueError("node_graph_csr needs nn >= 2, 0 < stride < nn, far_every >= 1, nfar >= 0 and excess > 0")
    rng = np.random.default_rng(seed)
    i = np.arange(nn)
    src, dst = [i[:-1], i[:-stride]], [i[1:], i[stride:]]
    far = i[::far_every]
    for _ in range(nfar):
        src.append(far)
        dst.append(rng.integers(0, nn, len(far)))
    s, d = np.concatenate(src), np.concatenate(dst)
    keep = s != d
    G = sp.coo_matrix((np.ones(int(keep.sum())), (s[keep], d[keep])), shape=(nn, nn)).tocsr()
    G = ((G + G.T) > 0).astype(np.float64) + sp.identity(nn, format="csr")
    A = sp.kron(G, np.ones((3, 3)), format="csr")
    A.sort_indices()
    A.data = -rng.random(A.nnz)
    A = sp.csr_matrix((A + A.T) * 0.5)
    A.sort_indices()
    rows = np.repeat(np.arange(3 * nn), np.diff(A.indptr))
    on_diag = A.indices == rows
    off = np.bincount(rows[~on_diag], weights=np.abs(A.data[~on_diag]), minlength=3 * nn)
    A.data[on_diag] = (1.0 + excess) * off
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), np.ascontiguousarray(A.data, dtype=np.float64)


def band_blocks_csr(blocks, seed, grading=0.0, shuffle=False, coupling=None):
    """Block-diagonal SPD matrix whose diagonal blocks have prescribed rows and bandwidth: `blocks` is a list of
    (rows b, bandwidth w), a w above b - 1 is clipped to b - 1.  Block q is L0 L0^T, symmetrised exactly (the upper
    triangle is the mirror of the lower one, bit for bit), L0 lower banded with every in-band entry nonzero:
    sub-diagonal magnitudes uniform in [0.25, 1] / sqrt(w + 1) with random sign, diagonal uniform in [1, 2] for
    grading = 0 and 10 ** U(-grading / 4, grading / 4) otherwise.  The band of the block is full and exactly w, so
    no ordering of it is narrower than the natural one.
    shuffle: a random symmetric permutation inside every block (the rows stay, the band does not).
    coupling = (per_row, mag): per_row random entries c, |c| uniform in [mag / 2, mag] with random sign, from every
    row to rows of other blocks, mirrored, with |c| added to both diagonal entries concerned: every such 2 x 2
    contribution is positive semidefinite and no entry inside a block other than its diagonal changes.
    Returns int32 rowptr, int32 colind, float64 val (sorted columns), the int32 part vector (rows of block q are
    contiguous and in part q) and the number of parts."""
    rng = np.random.default_rng(seed)
    blocks = [(int(b), min(int(w), int(b) - 1)) for b, w in blocks]
    if not blocks or any(b < 1 or w < 0 for b, w in blocks):
        raise ValueError("blocks must be a non-empty list of (rows >= 1, bandwidth >= 0)")
    P = len(blocks)
    N = sum(b for b, _ in blocks)
    rows, cols, vals = [], [], []
    r0 = 0
    for b, w in blocks:
        i, j = np.indices((b, b))
        inband = (i - j <= w) & (i > j)
        L0 = np.zeros((b, b))
        n = int(inband.sum())
        L0[inband] = rng.uniform(0.25, 1.0, n) / np.sqrt(w + 1.0) * rng.choice([-1.0, 1.0], n)
        if grading:
            L0[np.arange(b), np.arange(b)] = 10.0 ** rng.uniform(-grading / 4.0, grading / 4.0, b)
        else:
            L0[np.arange(b), np.arange(b)] = rng.uniform(1.0, 2.0, b)
        G = L0 @ L0.T
        A = np.tril(G) + np.tril(G, -1).T
        keep = np.abs(i - j) <= w
        if shuffle:
            p = rng.permutation(b)
            A, keep = A[np.ix_(p, p)], keep[np.ix_(p, p)]
        rows.append(r0 + i[keep])
        cols.append(r0 + j[keep])
        vals.append(A[keep])
        r0 += b
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    part = np.repeat(np.arange(P, dtype=np.int32), [b for b, _ in blocks])
    if coupling is not None:
        per_row, mag = int(coupling[0]), float(coupling[1])
        if P < 2:
            raise ValueError("coupling needs at least two blocks")
        ci = np.repeat(np.arange(N, dtype=np.int64), per_row)
        cj = rng.integers(0, N, ci.size)
        c = rng.uniform(0.5 * mag, mag, ci.size) * rng.choice([-1.0, 1.0], ci.size)
        other = part[ci] != part[cj]
        lo, hi, c = np.minimum(ci, cj)[other], np.maximum(ci, cj)[other], c[other]
        key, first = np.unique(lo * N + hi, return_index=True)          # one entry per pair of rows
        lo, hi, c = lo[first], hi[first], c[first]
        diag = np.zeros(N)
        np.add.at(diag, lo, np.abs(c))
        np.add.at(diag, hi, np.abs(c))
        vals[rows == cols] += diag[rows[rows == cols]]
        rows = np.concatenate([rows, lo, hi])
        cols = np.concatenate([cols, hi, lo])
        vals = np.concatenate([vals, c, c])
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=N))
    return rowptr.astype(np.int32), cols.astype(np.int32), np.ascontiguousarray(vals, dtype=np.float64), part, P
