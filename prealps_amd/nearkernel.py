"""Near-kernel vectors for EcgProblem.set_coarse_space, in the order and units of the caller's matrix."""
import numpy as np


def translations(N, dofs):
    """N x dofs: component c is 1 on the rows i with i % dofs == c (unknowns numbered node by node) -- the
    translations of an elasticity problem with `dofs` displacements per node; dofs = 1: the constant vector."""
    N, dofs = int(N), int(dofs)
    if dofs < 1 or N < 1:
        raise ValueError("translations(N, dofs) needs N >= 1 and dofs >= 1, not %d, %d" % (N, dofs))
    V = np.zeros((N, dofs), order="F")
    for c in range(dofs):
        V[c::dofs, c] = 1.0
    return V


def rigid_body_modes(coords):
    """coords: n x 3 node coordinates; returns 3n x 6 for unknowns (3 node + component): the three translations and
    the three rotations about the centroid, u = w x (x - x0) for w = e_x, e_y, e_z."""
    X = np.asarray(coords, dtype=np.float64)
    if X.ndim != 2 or X.shape[1] != 3:
        raise ValueError("coords must be n x 3, not of shape %r" % (X.shape,))
    n = X.shape[0]
    x, y, z = (X - X.mean(axis=0)).T
    V = np.zeros((3 * n, 6), order="F")
    V[0::3, 0] = V[1::3, 1] = V[2::3, 2] = 1.0
    V[1::3, 3], V[2::3, 3] = -z, y          # e_x x r = (0, -z, y)
    V[0::3, 4], V[2::3, 4] = z, -x          # e_y x r = (z, 0, -x)
    V[0::3, 5], V[1::3, 5] = -y, x          # e_z x r = (-y, x, 0)
    return V
