"""A numpy / plain-Python restatement of the reference's tree walk with ADAPTIVE_GRAVSOFT_FORGAS (test infrastructure).

The oracle (oracle/ngravs_oracle.c) has no adaptive softening, so the adaptive walk of the engine is held to this file, and this file
is held to the oracle first: with adaptive=False its tree (top-tree nodes of domain_determineTopTree included, force_create_empty_nodes
forcetree.c:292-336), moments, softening bits and walk are the oracle's, forces to 1e-12 and interaction counts equal
(tests/test_adaptive_softening.py pins that on the CPU).  The adaptive branch then differs in the softening lines alone:

  node     maxsoft, the largest softening length of anything below (forcetree.c:518-523, 600-601, 645-654, 705-709)
  pair     h = max(soft_i, soft_j), a gas particle's soft is its Hsml, any other's ForceSoftening[type] (:1398-1413, :1745-1760)
  opening  h = max(soft_target, maxsoft); the node is opened when soft_target < maxsoft and r2max < h^2, without the
           mixed-softening bit (:1503-1516, :1928-1941)

Empty nodes (no particle below: maxsofttype 7) are opened and not counted in both branches, as the engine handles them.
The lattice correction of periodic tree-only runs knows no softening: the tests add the oracle's own lattice walk.
"""
import math

import numpy as np

NTAB = 2048
TOPNODEFACTOR = 20.0   # domain.c:29
LAW_NONE, LAW_NEWTON, LAW_NEG_NEWTON, LAW_YUKAWA, LAW_COLOYUK = range(5)
SPLINE_NONE, SPLINE_PLUMMER, SPLINE_NEG_PLUMMER = range(3)


def law_accel(law, m, r2, r, ym):
    if law == LAW_NEWTON:
        return m / r2
    if law == LAW_NEG_NEWTON:
        return -m / r2
    if law == LAW_YUKAWA:
        return m * math.exp(-r * ym) * (ym / r + 1.0 / r2)
    if law == LAW_COLOYUK:
        return m * math.exp(-r * ym) * (ym / r + 1.0 / r2) + m / r2
    if law == LAW_NONE:
        return 0.0
    raise ValueError("law %d is not restated" % law)


def law_spline(sid, m, h, r):
    if sid == SPLINE_NONE:
        return 0.0
    if sid not in (SPLINE_PLUMMER, SPLINE_NEG_PLUMMER):
        raise ValueError("spline %d is not restated" % sid)
    h_inv = 1 / h
    u = r * h_inv
    if u < 0.5:
        v = m * h_inv * h_inv * h_inv * (10.666666666667 + u * u * (32.0 * u - 38.4))
    else:
        v = m * h_inv * h_inv * h_inv * (21.333333333333 - 48.0 * u + 38.4 * u * u - 10.666666666667 * u * u * u - 0.066666666667 / (u * u * u))
    return -v if sid == SPLINE_NEG_PLUMMER else v


def particle_soft(cfg, ptype, hsml):
    """the softening length of every particle under ADAPTIVE_GRAVSOFT_FORGAS"""
    fs = np.array([cfg.force_softening[t] for t in range(6)])
    soft = fs[np.asarray(ptype)]
    if hsml is not None:
        soft = np.where(np.asarray(ptype) == 0, np.asarray(hsml, dtype=np.float64), soft)
    return soft


class Node:
    __slots__ = ("ctr", "len", "kids", "m", "s", "mst", "diff", "maxsoft", "maxsoft_gas")


class Tree:
    """force_treebuild over the domain cube dom (Engine.domain() / O.domain_extent): dom[0:3] corner, [3:6] centre, [6] side,
    [7] = 2^bits / side"""

    def __init__(self, cfg, pos, mass, ptype, dom, hsml=None):
        self.cfg = cfg
        self.pos = np.ascontiguousarray(pos, dtype=np.float64)
        self.mass = np.ascontiguousarray(mass, dtype=np.float64)
        self.type = np.ascontiguousarray(ptype, dtype=np.int32)
        self.n = len(self.pos)
        self.ng = cfg.n_gravs
        self.fs = [cfg.force_softening[t] for t in range(6)]
        self.t2g = [cfg.type_to_grav[t] for t in range(6)]
        self.soft = particle_soft(cfg, self.type, hsml)
        self.gas = self.type == 0
        self.nodes = []
        dom = np.asarray(dom, dtype=np.float64)
        bits = int(round(math.log2(dom[7] * dom[6])))
        # integer coordinates as the keys see them (domain.c:938-944: the products are truncated to int)
        ic = ((self.pos - dom[0:3]) * dom[7]).astype(np.int64)
        self._ic, self._bits = ic, bits
        self._limit = self.n / TOPNODEFACTOR
        self.root = self._top(np.arange(self.n), [float(dom[3]), float(dom[4]), float(dom[5])], float(dom[6]), 0, True)
        self._moments(self.root)
        # plain lists for the walk
        self._P = self.pos.tolist()
        self._M = self.mass.tolist()
        self._T = self.type.tolist()
        self._S = self.soft.tolist()

    def _new(self, ctr, length):
        nd = Node()
        nd.ctr, nd.len, nd.kids = ctr, length, []
        self.nodes.append(nd)
        return len(self.nodes) - 1

    def _top(self, idx, ctr, length, depth, split):
        """a node of the top tree (domain_determineTopTree as the oracle restates it: the root is always split, a daughter when it
        holds more than N / TOPNODEFACTOR particles; all eight daughters become nodes, empty ones too)"""
        no = self._new(ctr, length)
        if not (split and depth < self._bits):
            self._fill(no, idx)
            return no
        sh = self._bits - depth - 1
        b = (self._ic[idx] >> sh) & 1
        slot = b[:, 0] + 2 * b[:, 1] + 4 * b[:, 2]
        for s in range(8):
            sub = idx[slot == s]
            c = [ctr[0] + (0.25 if s & 1 else -0.25) * length, ctr[1] + (0.25 if s & 2 else -0.25) * length,
                 ctr[2] + (0.25 if s & 4 else -0.25) * length]
            self.nodes[no].kids.append((s, self._top(sub, c, 0.5 * length, depth + 1, len(sub) > self._limit)))
        return no

    def _fill(self, no, idx):
        """particle insertion below a node (forcetree.c:150-250): an octant with one particle holds it directly, with more a node"""
        nd = self.nodes[no]
        if len(idx) == 0:
            return
        p = self.pos[idx]
        slot = (p[:, 0] > nd.ctr[0]).astype(np.int64) + 2 * (p[:, 1] > nd.ctr[1]) + 4 * (p[:, 2] > nd.ctr[2])
        for s in range(8):
            sub = idx[slot == s]
            if len(sub) == 1:
                nd.kids.append((s, -1 - int(sub[0])))       # a particle: -1 - index
            elif len(sub) > 1:
                half = 0.25 * nd.len
                c = [nd.ctr[0] + (half if s & 1 else -half), nd.ctr[1] + (half if s & 2 else -half), nd.ctr[2] + (half if s & 4 else -half)]
                ch = self._new(c, 0.5 * nd.len)
                nd.kids.append((s, ch))
                self._fill(ch, sub)

    def _merge_soft(self, nd, ty, tdiff):
        """force_update_node_recursive's maxsofttype / diffsoftflag (forcetree.c:556-600, 655-700)"""
        nd.diff |= tdiff
        if ty == 7:
            return
        if nd.mst == 7:
            nd.mst = ty
        elif self.fs[ty] > self.fs[nd.mst]:
            nd.mst = ty
            nd.diff = 1
        elif self.fs[ty] < self.fs[nd.mst]:
            nd.diff = 1

    def _moments(self, no):
        nd = self.nodes[no]
        ng = self.ng
        m = [0.0] * ng
        s = [[0.0, 0.0, 0.0] for _ in range(ng)]
        nd.mst, nd.diff, nd.maxsoft, nd.maxsoft_gas = 7, 0, 0.0, False
        for _, k in nd.kids:
            if k >= 0:
                self._moments(k)
                c = self.nodes[k]
                for g in range(ng):
                    m[g] += c.m[g]
                    for j in range(3):
                        s[g][j] += c.m[g] * c.s[g][j]
                self._merge_soft(nd, c.mst, c.diff)
                if c.maxsoft > nd.maxsoft:
                    nd.maxsoft, nd.maxsoft_gas = c.maxsoft, c.maxsoft_gas
            else:
                p = -1 - k
                ty = int(self.type[p])
                g = self.t2g[ty]
                m[g] += float(self.mass[p])
                for j in range(3):
                    s[g][j] += float(self.mass[p]) * float(self.pos[p, j])
                self._merge_soft(nd, ty, 0)
                if self.soft[p] > nd.maxsoft:
                    nd.maxsoft, nd.maxsoft_gas = float(self.soft[p]), bool(self.gas[p])
        for g in range(ng):
            if m[g] > 0:
                s[g] = [s[g][0] / m[g], s[g][1] / m[g], s[g][2] / m[g]]
            else:
                s[g] = list(nd.ctr)
        nd.m, nd.s = m, s

    # ---- force_treeevaluate / force_treeevaluate_shortrange, mode 0 ---------------------------------------------------------
    def walk(self, idx=None, old_acc=None, table=None, adaptive=False, cfg=None):
        """-> acc [nt][3] (without G), nint [nt], A [nt], B [nt].  A: node visits opened by the softening rule alone; B: pair
        interactions (a particle or a node against the target, the target itself excluded) with r < h where h is a gas
        particle's length"""
        cfg = cfg if cfg is not None else self.cfg
        idx = np.arange(self.n) if idx is None else np.asarray(idx)
        ng, pm, periodic = self.ng, cfg.pmgrid != 0, cfg.periodic != 0
        box, boxhalf = cfg.box_size, 0.5 * cfg.box_size
        theta2 = cfg.err_tol_theta * cfg.err_tol_theta
        use_theta = cfg.err_tol_theta != 0
        ym = cfg.yukawa_imass / cfg.box_size if cfg.box_size > 0 else 0.0
        la = [[cfg.law_accel[i][j] for j in range(ng)] for i in range(ng)]
        ls = [[cfg.law_spline[i][j] for j in range(ng)] for i in range(ng)]
        rcut = rcut2 = asmthfac = utor2wpi = 0.0
        if pm:
            asmth = cfg.asmth if cfg.asmth > 0 else 1.25 * cfg.box_size / cfg.pmgrid
            rcut = cfg.rcut if cfg.rcut > 0 else 4.5 * asmth
            rcut2 = rcut * rcut
            asmthfac = 0.5 / asmth * (NTAB / 3.0)
            utor2wpi = 1.0 / (math.pi * 4 * asmth * asmth)
            table = np.asarray(table, dtype=np.float64).reshape(ng, ng, NTAB)
        P, M, T, S, fs, t2g, nodes = self._P, self._M, self._T, self._S, self.fs, self.t2g, self.nodes
        gas = self.gas.tolist()
        acc = np.zeros((len(idx), 3))
        nint = np.zeros(len(idx), dtype=np.int64)
        cA = np.zeros(len(idx), dtype=np.int64)
        cB = np.zeros(len(idx), dtype=np.int64)

        def nearest(x):
            return x - box if x > boxhalf else (x + box if x < -boxhalf else x)

        for k, t in enumerate(idx.tolist()):
            px, py, pz = P[t]
            ptype = T[t]
            tg = t2g[ptype]
            soft_t = S[t] if adaptive else fs[ptype]
            t_gas = adaptive and gas[t]
            aold = cfg.err_tol_force_acc * (float(old_acc[t]) if old_acc is not None else 0.0)
            st = [0.0, 0.0, 0.0, 0, 0, 0]   # ax, ay, az, nint, A, B

            def interact(g, dx, dy, dz, r2, m, h):
                r = math.sqrt(r2)
                if pm:
                    tab = int(asmthfac * r)
                    if tab >= NTAB:
                        return False
                    if r >= h:
                        fac = law_accel(la[tg][g], m, r2, r, ym)
                        fac -= m * utor2wpi * table[tg, g, tab]
                        fac /= r
                    else:
                        fac = law_spline(ls[tg][g], m, h, r)
                elif r >= h:
                    fac = law_accel(la[tg][g], m, r2, r, ym) / r
                else:
                    fac = law_spline(ls[tg][g], m, h, r)
                st[0] += dx * fac
                st[1] += dy * fac
                st[2] += dz * fac
                return True

            def particle(p):
                qt = T[p]
                dx, dy, dz = P[p][0] - px, P[p][1] - py, P[p][2] - pz
                if periodic:
                    dx, dy, dz = nearest(dx), nearest(dy), nearest(dz)
                r2 = dx * dx + dy * dy + dz * dz
                h = soft_t
                from_gas = t_gas
                hq = S[p] if adaptive else fs[qt]
                if h < hq:
                    h = hq
                    from_gas = adaptive and gas[p]
                added = interact(t2g[qt], dx, dy, dz, r2, M[p], h)
                if added or not pm:
                    st[3] += 1
                if added and p != t and from_gas and math.sqrt(r2) < h:
                    st[5] += 1

            def visit(no):
                nd = nodes[no]
                dx, dy, dz, r2 = [0.0] * ng, [0.0] * ng, [0.0] * ng, [0.0] * ng
                r2min, r2max, summass = math.inf, -math.inf, 0.0
                for g in range(ng):
                    summass += nd.m[g]
                    x, y, z = nd.s[g][0] - px, nd.s[g][1] - py, nd.s[g][2] - pz
                    if periodic:
                        x, y, z = nearest(x), nearest(y), nearest(z)
                    dx[g], dy[g], dz[g] = x, y, z
                    r2[g] = x * x + y * y + z * z
                    r2min = min(r2min, r2[g])
                    r2max = max(r2max, r2[g])
                ln = nd.len
                if pm and r2min > rcut2:
                    eff = rcut + 0.5 * ln
                    for j, q in enumerate((px, py, pz)):
                        d = nd.ctr[j] - q
                        if periodic:
                            d = nearest(d)
                        if d < -eff or d > eff:
                            return
                opened = False
                if use_theta:
                    opened = ln * ln > r2min * theta2
                else:
                    opened = summass * ln * ln > r2min * r2min * aold
                    if not opened:
                        opened = abs(nd.ctr[0] - px) < 0.60 * ln and abs(nd.ctr[1] - py) < 0.60 * ln and abs(nd.ctr[2] - pz) < 0.60 * ln
                h = soft_t
                from_gas = t_gas
                if not opened:
                    if nd.mst == 7:
                        assert summass == 0
                        opened = True
                    elif adaptive:
                        if h < nd.maxsoft:
                            h = nd.maxsoft
                            from_gas = nd.maxsoft_gas
                            if r2max < h * h:
                                opened = True
                                st[4] += 1
                    elif h < fs[nd.mst]:
                        h = fs[nd.mst]
                        if r2max < h * h and nd.diff:
                            opened = True
                            st[4] += 1
                if opened:
                    for _, c in nd.kids:
                        if c >= 0:
                            visit(c)
                        else:
                            particle(-1 - c)
                    return
                added = False
                for g in range(ng):
                    if nd.m[g] != 0.0:
                        a = interact(g, dx[g], dy[g], dz[g], r2[g], nd.m[g], h)
                        added = added or a
                        if a and from_gas and math.sqrt(r2[g]) < h:
                            st[5] += 1
                if added or not pm:
                    st[3] += 1

            visit(self.root)
            acc[k] = st[0:3]
            nint[k], cA[k], cB[k] = st[3], st[4], st[5]
        return acc, nint, cA, cB


def lattice_lookup(tab, box, dx, dy, dz):
    """lattice_corr (forcetree.c:3803-3885) for arrays of separations: tab [3][65][65][65] -> [n][3]"""
    EN = tab.shape[1] - 1
    fac = 2 * EN / box
    d = np.stack([dx, dy, dz], axis=1)
    sg = np.where(d < 0, 1.0, -1.0)
    u = np.abs(d) * fac
    i = np.minimum(u.astype(np.int64), EN - 1)
    u = u - i
    out = np.zeros_like(d)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                w = (u[:, 0] if a else 1 - u[:, 0]) * (u[:, 1] if b else 1 - u[:, 1]) * (u[:, 2] if c else 1 - u[:, 2])
                for comp in range(3):
                    out[:, comp] += tab[comp, i[:, 0] + a, i[:, 1] + b, i[:, 2] + c] * w
    return sg * out


def direct(cfg, pos, mass, ptype, soft, idx, lat=None):
    """the plain double loop with h = max(soft_i, soft_j) (force_treeevaluate_direct, forcetree.c:3428-3548, with the pair rule
    of :1398-1413); periodic: nearest image, plus the lattice tables lat [tg][sg][3][65^3] where u > 1e-5.  -> acc * G"""
    pos, mass, ptype, soft = np.asarray(pos, dtype=np.float64), np.asarray(mass, dtype=np.float64), np.asarray(ptype), np.asarray(soft)
    ng = cfg.n_gravs
    t2g = np.array([cfg.type_to_grav[t] for t in range(6)])
    sg_all = t2g[ptype]
    box, boxhalf = cfg.box_size, 0.5 * cfg.box_size
    ym = cfg.yukawa_imass / cfg.box_size if cfg.box_size > 0 else 0.0
    out = np.zeros((len(idx), 3))
    for k, t in enumerate(np.asarray(idx).tolist()):
        tg = t2g[ptype[t]]
        d = pos - pos[t]
        if cfg.periodic:
            d = np.where(d > boxhalf, d - box, np.where(d < -boxhalf, d + box, d))
        r2 = np.einsum("ij,ij->i", d, d)
        r = np.sqrt(r2)
        h = np.maximum(soft, soft[t])
        u = r * (1 / h)
        fac = np.zeros(len(pos))
        for g in range(ng):
            law, sid = cfg.law_accel[tg][g], cfg.law_spline[tg][g]
            far = (sg_all == g) & (u >= 1)
            near = (sg_all == g) & ~(u >= 1)
            m, rr, rr2 = mass[far], r[far], r2[far]
            if law in (LAW_NEWTON, LAW_NEG_NEWTON):
                f = m / rr2 * (1.0 if law == LAW_NEWTON else -1.0)
            elif law in (LAW_YUKAWA, LAW_COLOYUK):
                f = m * np.exp(-rr * ym) * (ym / rr + 1.0 / rr2) + (m / rr2 if law == LAW_COLOYUK else 0.0)
            elif law == LAW_NONE:
                f = np.zeros(len(m))
            else:
                raise ValueError("law %d is not restated" % law)
            fac[far] = f / rr
            if sid != SPLINE_NONE:
                hi = 1 / h[near]
                x = r[near] * hi
                with np.errstate(divide="ignore", invalid="ignore"):
                    v = np.where(x < 0.5, 10.666666666667 + x * x * (32.0 * x - 38.4),
                                 21.333333333333 - 48.0 * x + 38.4 * x * x - 10.666666666667 * x * x * x - 0.066666666667 / (x * x * x))
                fac[near] = mass[near] * hi * hi * hi * v * (-1.0 if sid == SPLINE_NEG_PLUMMER else 1.0)
        a = (d * fac[:, None]).sum(axis=0)
        if lat is not None:
            for g in range(ng):
                sel = (sg_all == g) & (u > 1.0e-5)
                a += (lattice_lookup(lat[tg, g], box, d[sel, 0], d[sel, 1], d[sel, 2]) * mass[sel, None]).sum(axis=0)
        out[k] = a * cfg.G
    return out


# ---- the input sets of tests/test_adaptive_softening.py ------------------------------------------------------------------------
def gas_lengths(pos_gas, rng, box=0.0):
    """distance to the 32nd nearest gas particle times a seeded factor in [0.5, 2]"""
    n = len(pos_gas)
    out = np.zeros(n)
    for i in range(n):
        d = pos_gas - pos_gas[i]
        if box > 0:
            d -= box * np.rint(d / box)
        r = np.sqrt(np.einsum("ij,ij->i", d, d))
        out[i] = np.partition(r, 32)[32]
    return out * rng.uniform(0.5, 2.0, n)


def mixed_types(n_gas, n1, n2, rng):
    typ = np.concatenate([np.zeros(n_gas), np.ones(n1), np.full(n2, 2)]).astype(np.int32)
    return typ[rng.permutation(len(typ))]
