"""NumPy restatement of the recursion pgas_amd.ModelRollout runs on the device, for the tests:

    v_i   = feature_i(x_t, u_t)                     a pick of concat(x_t, u_t), or a callable such as the Vehicle's slip angles
    phi_i = Hilbert basis of v_i                    (src/BasisFunctions.py:77-80)
    xi_i  = A_k,i phi_i [+ e Lrow^T]
    y_t   = g(x_t, u_t, xi),    x_t+1 = f(x_t, u_t, xi) [+ z Qc^T]

with step t -> t+1 reading input row t, as the reference's validation loop (src/EMPS.py:129-151) and Algorithm1 do.  Written from the
formulas, not from the package's batched helpers; random numbers come in as arrays.
"""
from __future__ import annotations

import numpy as np


class Latent:
    """basis: a pgas_amd BasisMap or an object with `feature(xp)` and a BasisMap `map` (its tables are read, not its methods)."""

    def __init__(self, basis):
        b = getattr(basis, "b", basis)
        self.fn = b.feature(np) if hasattr(b, "feature") else None
        self.map = b.map if self.fn is not None else b

    def argument(self, x, u):
        if self.fn is not None:
            return self.fn(x, u)[:, self.map.sel]
        v = x if not np.size(u) else np.concatenate([x, np.broadcast_to(np.reshape(u, (1, -1)), (x.shape[0], np.size(u)))], axis=1)
        return v[:, self.map.sel]

    def phi(self, x, u):
        b = self.map.basis
        w = (self.argument(x, u) / self.map.div - b.center + b.L) / b.size                       # (P, D)
        return np.prod(np.sqrt(1.0 / b.L) * np.sin(np.pi * b.indices[None, :, :] * w[:, None, :]), axis=2)   # (P, M)


def step(model, latents, A, x, u, z=None, Qc=None, e=None, Lrow=None):
    """One step for P replicates of one draw: A list of (n_i, M_i), x (P, nx), u (nu,) -> (xi list of (P, n_i), y (P, ny), x_next (P, nx)).
    The coefficient product is taken replicate by replicate, (n, M) @ (M,), as the reference's loop takes it."""
    f, g = model
    xi = []
    for i, lat in enumerate(latents):
        phi = lat.phi(x, u)
        m = np.stack([A[i] @ phi[p] for p in range(x.shape[0])])
        if e is not None:
            m = m + e[i] @ Lrow[i].T
        xi.append(m)
    y = g(x, u, *xi)
    xn = f(x, u, *xi)
    if z is not None:
        xn = xn + z @ Qc.T
    return xi, y.reshape(x.shape[0], -1), xn


def rollout(model, latents, A, inputs, x0, z=None, Qc=None):
    """A: list of (K, n_i, M_i); inputs (T, nu); x0 (K, P, nx); z (K, T, P, nx) with z[:, t] the normals of time index t (row 0 unused)
    -> out_x (K, T, P, nx), out_y (K, T, P, ny)."""
    K, P, nx = x0.shape
    T = inputs.shape[0]
    out_x, out_y = np.zeros((K, T, P, nx)), None
    for k in range(K):
        x = x0[k]
        out_x[k, 0] = x
        for t in range(T):
            _, y, xn = step(model, latents, [a[k] for a in A], x, inputs[t], None if z is None or t == T - 1 else z[k, t + 1], Qc)
            if out_y is None:
                out_y = np.zeros((K, T, P, y.shape[1]))
            out_y[k, t] = y
            if t < T - 1:
                out_x[k, t + 1] = x = xn
    return out_x, out_y
