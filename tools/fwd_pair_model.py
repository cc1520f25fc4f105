#!/usr/bin/env python3
"""Lane-level numpy model of riccati_forward_kernel (robotoc_amd/csrc/riccati_forward.hpp), the one-wave forward Riccati
recursion with the row-pair x column-group lane map.

The kernel reads every matrix of a grid point with 16-byte loads: lane l = c * NV + p (l < G * NV, G = 64 // NV) owns row
pair p and column group c and takes, in load t, rows 2p, 2p+1 of column G t + c.  Its partial sums go through LDS and are
reduced in a fixed order.  This file states that algebra on flat records with explicit 64-lane arrays: the addresses of
every load (in doubles from the field start), the lane-local sums in load order, the reduction over c (Fxx dx, P dx) and
over p (K dx), the flat Fvu copy, and the row sums of the tail.  P of a grid point i < N is read from its lower triangle
only (p_pair_live, sym_matvec_partials, sym_reduce_rows: own-row terms over c, mirror terms over p); the terminal P in
full.  forward_instance() runs it over a whole grid and returns
the direction records; tests/test_fwd_pair_model.py holds it against the oracle's forward recursion for every one-wave
shape, trot and jump-STO grids included.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from robotoc_amd.types import GRID_IMPACT, GRID_LIFT, Records  # noqa: E402

LANES = np.arange(64)


class LaneMap:
    """FwdPairCfg<NV, NU, NS> and the lane roles of the kernel."""

    def __init__(self, nv, nu):
        self.nv, self.nu, self.nx = nv, nu, 2 * nv
        assert 2 * nv + nu <= 64
        self.G = 64 // nv
        self.TX = -(-self.nx // self.G)
        self.TK = -(-nu // self.G)
        self.NF = nv * nu
        self.TF = -(-(self.NF + (self.NF & 1)) // 128)
        self.lg = LANES < self.G * nv
        self.p = np.where(self.lg, LANES % nv, LANES - self.G * nv)
        self.c = np.where(self.lg, LANES // nv, 0)

    def moff(self, t):
        """Offset (doubles) of each lane's 16 bytes in load t of an NX x NX column-major matrix, and whether it counts."""
        j = self.G * t + self.c
        live = j < self.nx
        return np.where(live, j * self.nx + 2 * self.p, (self.nx - 1) * self.nx + 2 * self.p), live

    def koff(self, t):
        """The same for K (row-major nu x nx = K^T column-major): row u = G t + c."""
        u = self.G * t + self.c
        live = u < self.nu
        return np.where(live, u * self.nx + 2 * self.p, (self.nu - 1) * self.nx + 2 * self.p), live, u


def pair_load(field, off):
    """global_load_dwordx4: lane l gets field[off[l]], field[off[l] + 1]."""
    return field[off], field[off + 1]


def matvec_partials(m, A, dx):
    """Per-lane sums over the lane's columns of A (flat, column-major NX x NX) times dx, in load order."""
    a0 = np.zeros(64)
    a1 = np.zeros(64)
    for t in range(m.TX):
        off, live = m.moff(t)
        x = np.where(live, dx[np.minimum(m.G * t + m.c, m.nx - 1)], 0.0)  # the permuted copy holds 0 past NX
        lo, hi = pair_load(A, off)
        a0 = np.where(live, a0 + lo * x, a0)
        a1 = np.where(live, a1 + hi * x, a1)
    return a0, a1


def reduce_rows(m, a0, a1):
    """sPa[c][2p..2p+1] written by lanes l < G NV; lane r < NX sums sPa[0..G-1][r] in order of c."""
    part = np.zeros((m.G, m.nx))
    for l in range(m.G * m.nv):
        part[m.c[l], 2 * m.p[l]] = a0[l]
        part[m.c[l], 2 * m.p[l] + 1] = a1[l]
    out = part[0].copy()
    for c in range(1, m.G):
        out = out + part[c]
    return out


def k_times_dx(m, K, dx):
    """K dx: lane (p, c) forms K[u][2p] dx[2p] + K[u][2p+1] dx[2p+1] for u = G t + c; lane NX + u sums over p in order."""
    part = np.zeros((m.nu, m.nv))
    for t in range(m.TK):
        off, live, u = m.koff(t)
        lo, hi = pair_load(K, off)
        pk = lo * dx[2 * m.p] + hi * dx[2 * m.p + 1]
        for l in range(m.G * m.nv):
            if live[l]:
                part[u[l], m.p[l]] = pk[l]
    out = np.zeros(m.nu)
    for p in range(m.nv):
        out = out + part[:, p]
    return out


def p_pair_live(m, t):
    """Which lanes request their pair of load t of P at a grid point i < N: the pair reaches the diagonal, 2p + 1 >= j.
    Lanes past G NV and columns past the matrix are silent (2p + 1 < NX)."""
    j = m.G * t + m.c
    return m.lg & (2 * m.p + 1 >= j)


def p_live_pairs(m):
    """(live, all) 16-B pairs of one P: what the lower triangle takes of the full walk."""
    return sum(int(p_pair_live(m, t).sum()) for t in range(m.TX)), m.nx * m.nv


def sym_matvec_partials(m, P, dx):
    """P dx from the lower triangle of a symmetric P (flat, column-major).  A live pair gives P[2p][j] x[j] (2p >= j) and
    P[2p+1][j] x[j] to its own rows, summed over the lane's loads in order, and the mirror terms P[2p][j] x[2p] (2p > j)
    + P[2p+1][j] x[2p+1] (2p + 1 > j) to row j: mir[j][p], a partial over p.  Silent lanes read nothing (the buffer load
    returns zero); every term is selected, so an element above the diagonal -- the upper one of a pair astride it --
    never enters a sum."""
    q0 = np.zeros(64)
    q1 = np.zeros(64)
    mir = np.zeros((m.nx, m.nv))
    x0, x1 = dx[2 * m.p], dx[2 * m.p + 1]
    for t in range(m.TX):
        j = m.G * t + m.c
        live = p_pair_live(m, t)
        dd = np.where(m.lg, j - 2 * m.p, 1 << 20)
        off = np.where(live, j * m.nx + 2 * m.p, 0)
        lo, hi = pair_load(P, off)
        lo, hi = np.where(live, lo, 0.0), np.where(live, hi, 0.0)
        xt = dx[np.minimum(j, m.nx - 1)]
        q0 = np.where(dd <= 0, q0 + lo * xt, q0)
        q1 = np.where(dd <= 1, q1 + hi * xt, q1)
        m1 = hi * x1
        m01 = m1 + lo * x0
        mv = np.where(dd < 0, m01, np.where(dd < 1, m1, 0.0))
        for l in range(m.G * m.nv):
            if j[l] < m.nx:
                mir[j[l], m.p[l]] = mv[l]
    return q0, q1, mir


def sym_reduce_rows(m, q0, q1, mir):
    """Row sums of P dx: the own-row partials over c as reduce_rows, then the mirror partials of the row over p in order."""
    acc = np.zeros(m.nx)
    for p in range(m.nv):
        acc = acc + mir[:, p]
    return reduce_rows(m, q0, q1) + acc


def fvu_copy(m, Fvu_field):
    """The flat 16-B copy of Fvu into LDS (an odd NV NU reads one double of the field's padding, never used)."""
    sF = np.zeros(m.TF * 128)
    for i in range(m.TF):
        e = 2 * (64 * i + LANES)
        src = np.where(e < m.NF, e, 0)
        lo, hi = pair_load(Fvu_field, src)
        sF[e] = lo
        sF[e + 1] = hi
    return sF


def forward_instance(L, grids, kkt, ric, dx0):
    """dir records [stages, stride] of one instance from its kkt and ric records, the kernel's order of operations."""
    K_, R_, D_ = Records(L, "kkt"), Records(L, "ric"), Records(L, "dir")
    nv, nu, ns = L.dims.nv, L.dims.nu, L.dims.ns_max
    m = LaneMap(nv, nu)
    nx = m.nx
    n = len(grids)
    N = n - 1
    d = D_.zeros(n)
    sz = lambda R, name: int(np.prod(R.shapes[name]))
    fk = lambda st, name: kkt[st, K_.offset(name):K_.offset(name) + sz(K_, name)]
    fr = lambda st, name: ric[st, R_.offset(name):R_.offset(name) + sz(R_, name)]
    fd = lambda st, name: d[st, D_.offset(name):D_.offset(name) + sz(D_, name)]
    # padded fields: the 16-B loads may read one double past a field of odd length
    fkp = lambda st, name: kkt[st, K_.offset(name):K_.offset(name) + sz(K_, name) + 1]
    dx = dx0.astype(np.float64).copy()
    fd(0, "dx")[:] = dx
    dts = dtsn = 0.0
    if grids[0].sto:
        acc = 0.0
        for k in range(nx):
            acc += fr(0, "dtsdx")[k] * dx[k]
        dtsn = acc + fr(0, "scal")[6]
    for st in range(N):
        g = grids[st]
        impact, lift = g.type == GRID_IMPACT, g.type == GRID_LIFT
        if impact or lift:
            dts, dtsn = dtsn, 0.0
            if lift and g.sto_next:
                acc = 0.0
                for k in range(nx):
                    acc += fr(st, "dtsdx")[k] * dx[k]
                acc += fr(st, "scal")[6]
                if g.sto:
                    acc += fr(st, "scal")[5] * dts
                dtsn = acc
        acc_a = reduce_rows(m, *matvec_partials(m, fk(st, "Fxx"), dx))
        acc_p = sym_reduce_rows(m, *sym_matvec_partials(m, fr(st, "P"), dx))   # i < N: the lower triangle only
        dxn = fk(st, "Fx") + acc_a
        if not impact:
            du = k_times_dx(m, fr(st, "K"), dx) + fr(st, "k")
            if g.sto:
                du = du + fr(st, "T") * (dtsn - dts)
                if g.sto_next:
                    du = du - fr(st, "W") * dtsn
            fd(st, "du")[:] = du
            sF = fvu_copy(m, fkp(st, "Fvu"))
            for r in range(nv, nx):
                v = dxn[r]
                for cc in range(nu):
                    v += sF[cc * nv + r - nv] * du[cc]
                dxn[r] = v
            if g.sto:
                dxn = dxn + fk(st, "fx") * (dtsn - dts)
        fd(st + 1, "dx")[:] = dxn
        if impact and g.sto_next:
            acc = 0.0
            for k in range(nx):
                acc += fr(st, "dtsdx")[k] * dxn[k]
            acc += fr(st, "scal")[6]
            if g.sto:
                acc += fr(st, "scal")[5] * dts
            dtsn = acc
        lam = acc_p - fr(st, "s")
        if g.sto:
            if impact:
                lam = lam - fr(st, "Phi") * dtsn
            else:
                lam = lam + fr(st, "Psi") * (dtsn - dts)
                if g.sto_next:
                    lam = lam - fr(st, "Phi") * dtsn
        fd(st, "dlmdgmm")[:] = lam
        if ns > 0 and g.switching_constraint:
            M = fr(st, "M")
            for i in range(g.dims):
                acc = 0.0
                for j in range(nx):
                    acc += M[j * ns + i] * dx[j]
                acc += fr(st, "m")[i]
                if g.sto:
                    acc += fr(st, "mt")[i] * (dtsn - dts)
                    if g.sto_next:
                        acc -= fr(st, "mt_next")[i] * dtsn
                fd(st, "dxi")[i] = acc
        fd(st, "dts")[0] = dts
        fd(st, "dts")[1] = dtsn
        dx = dxn
    fd(N, "dlmdgmm")[:] = reduce_rows(m, *matvec_partials(m, fr(N, "P"), dx)) - fr(N, "s")
    fd(N, "dts")[0] = dts
    fd(N, "dts")[1] = dtsn
    return d
