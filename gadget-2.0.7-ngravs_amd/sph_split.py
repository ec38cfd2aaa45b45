"""density() and hydro_force() over a particle set that is split over several engines of ONE process: the reference's export loop
(density.c:120-290, hydra.c:118-300) with engines in the place of tasks.

This is the per-task half of SPH across tasks put to work without a communicator: every engine holds its own particles and its
own tree; a target's sums are taken on its own engine first (Engine.sph_density_sums / sph_hydro_sums, the reference's
density_evaluate(i, 0)), then on every other engine the export decision names, in ascending engine index (density_evaluate(j, 1)
on the importing task); the owner adds them and finishes them (sph_density_update; hydra.c:320).  The drivers over the
communicator vtable and the glue replace the Python loops below by exchanges; what an engine computes stays the same.

The export decision is a pure numpy function.  The reference exports to the tasks whose top-level tree leaves the search box
touches (ngb.c:272-297 on pseudo-particles); here a target goes to engine b when its search box overlaps the bounding box of b's
gas, periodic images included.  It has to be a superset of the engines that hold a neighbour, nothing more: an engine that gets
a target it has no neighbour for returns zeros.
"""
import numpy as np

from . import NgravsError, sph_density_update

DENS_KEYS = ("hsml", "density", "num_ngb", "div_vel", "curl_vel", "dhsml_factor")
HYDRO_COLS = ("hsml", "density", "pressure", "dhsml_factor", "div_vel", "curl_vel")


class Task:
    """one engine and the host columns of its last hand-over (the engine keeps them on the device only)"""

    def __init__(self, engine, pos, mass, ptype, active=None):
        self.engine = engine
        self.set_columns(pos, mass, ptype, active)

    def set_columns(self, pos, mass, ptype, active=None):
        self.pos = np.ascontiguousarray(pos, dtype=np.float64)
        self.mass = np.ascontiguousarray(mass, dtype=np.float64)
        self.ptype = np.ascontiguousarray(ptype, dtype=np.int32)
        self.active = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)

    def update_particles(self, pos, active=None):
        """drifted positions / new active flags: Engine.update_particles (the tree is refit by the next SPH call)"""
        self.engine.update_particles(pos, self.mass, self.ptype, active=active)
        self.set_columns(pos, self.mass, self.ptype, active)

    @property
    def box(self):
        return float(self.engine.cfg.box_size) if self.engine.cfg.periodic else 0.0

    def gas(self):
        return np.nonzero(self.ptype == 0)[0]

    def targets(self):
        """active type-0 rows (density.c:95, :123)"""
        t = self.ptype == 0
        if self.active is not None:
            t &= (self.active & 1) != 0
        return np.nonzero(t)[0]

    def gas_bounds(self, hsml=None):
        """(lo[3], hi[3], largest Hsml) of the gas; None for an engine without gas"""
        g = self.gas()
        if not len(g):
            return None
        return self.pos[g].min(axis=0), self.pos[g].max(axis=0), 0.0 if hsml is None else float(np.max(np.asarray(hsml)[g]))


def box_overlap(tpos, radius, lo, hi, box=0.0):
    """bool [nt]: the search box tpos +- radius overlaps [lo, hi]; periodic (box > 0): some image of it does"""
    tpos = np.asarray(tpos, dtype=np.float64).reshape(-1, 3)
    radius = np.broadcast_to(np.asarray(radius, dtype=np.float64), (len(tpos),))
    ok = np.ones(len(tpos), dtype=bool)
    for k in range(3):
        hit = np.zeros(len(tpos), dtype=bool)
        for shift in ((-box, 0.0, box) if box else (0.0,)):
            x = tpos[:, k] + shift
            hit |= (x - radius <= hi[k]) & (x + radius >= lo[k])
        ok &= hit
    return ok


def density_export(tpos, th, bounds, box=0.0):
    """bool [nt, engines]: the engines a density target is summed on: search box pos +- h against the bounding box of an
    engine's gas.  bounds: Task.gas_bounds() per engine."""
    out = np.zeros((len(tpos), len(bounds)), dtype=bool)
    for b, bd in enumerate(bounds):
        if bd is not None:
            out[:, b] = box_overlap(tpos, th, bd[0], bd[1], box)
    return out


def hydro_export(tpos, th, bounds, box=0.0):
    """bool [nt, engines]: as density_export with the radius max(h, largest Hsml of the engine's gas): the pair test of
    hydra.c:436 is r < h_i or r < h_j"""
    out = np.zeros((len(tpos), len(bounds)), dtype=bool)
    for b, bd in enumerate(bounds):
        if bd is not None:
            out[:, b] = box_overlap(tpos, np.maximum(th, bd[2]), bd[0], bd[1], box)
    return out


def export_everywhere(tpos, th, bounds, box=0.0):
    """every target to every engine: what the results must not depend on"""
    return np.ones((len(tpos), len(bounds)), dtype=bool)


def density_over(tasks, vel, hsml, des_num_ngb, max_num_ngb_deviation, min_gas_hsml=0.0, export=density_export):
    """density() of the reference over the engines of `tasks`.  vel, hsml: one array per task (SphP[].VelPred [n,3], starting
    guesses [n]).  Per round every task's unconverged targets are summed on their own engine, then on the engines `export`
    names in ascending index; the sums are added, sph_density_update decides.  Returns one dict per task: hsml, density, num_ngb,
    div_vel, curl_vel, dhsml_factor over its rows (rows that are no targets: the given hsml, else 0), rounds (int32 [n]) and
    max_rounds, the most rounds any target of any task took.  MAXITER raises NgravsError as Engine.sph_density does."""
    vel = [np.ascontiguousarray(v, dtype=np.float64) for v in vel]
    box = tasks[0].box
    bounds = [t.gas_bounds() for t in tasks]
    res, state = [], []
    for a, t in enumerate(tasks):
        n = len(t.pos)
        r = {k: np.zeros(n) for k in DENS_KEYS}
        r["hsml"] = np.array(hsml[a], dtype=np.float64)
        r["rounds"] = np.zeros(n, dtype=np.int32)
        res.append(r)
        rows = t.targets()
        state.append(dict(rows=rows, h=r["hsml"][rows].copy(), left=np.zeros(len(rows)), right=np.zeros(len(rows)),
                          rounds=np.zeros(len(rows), dtype=np.int32)))
    while any(len(s["rows"]) for s in state):
        for a, t in enumerate(tasks):
            s = state[a]
            rows = s["rows"]
            if not len(rows):
                continue
            tpos, tvel, th = t.pos[rows], vel[a][rows], s["h"]
            sums = t.engine.sph_density_sums(vel[a], tpos, tvel, th)             # density_evaluate(i, 0)
            mask = export(tpos, th, bounds, box)
            for b, other in enumerate(tasks):
                sel = np.nonzero(mask[:, b])[0] if b != a else ()
                if len(sel):                                                      # density_evaluate(j, 1) on task b
                    sums[sel] += other.engine.sph_density_sums(vel[b], tpos[sel], tvel[sel], th[sel])
            s["sums"] = sums
        for a, t in enumerate(tasks):                                             # the owners' side
            s = state[a]
            rows = s["rows"]
            if not len(rows):
                continue
            up = sph_density_update(s["sums"], s["h"], s["left"], s["right"], s["rounds"], des_num_ngb, max_num_ngb_deviation, min_gas_hsml)
            if up["failed"]:
                raise NgravsError("density_over failed: status -4 (failed to converge in neighbour iteration in density())")   # endrun(1155)
            acc = up["accepted"] != 0
            for k in DENS_KEYS:
                res[a][k][rows[acc]] = up[k][acc]
            res[a]["rounds"][rows[acc]] = s["rounds"][acc]
            keep = ~acc
            state[a] = dict(rows=rows[keep], h=s["h"][keep], left=s["left"][keep], right=s["right"][keep], rounds=s["rounds"][keep])
    most = max([int(r["rounds"].max()) if len(r["rounds"]) else 0 for r in res] + [0])
    for r in res:
        r["max_rounds"] = most
    return res


def hydro_targets(task, vel, col, rows, timestep=None, gamma=5.0 / 3, fac_mu=1.0):
    """the reference's hydrodata_in (hydra.c:145-162) for the rows `rows` of a task: what its owner sends, F1 included"""
    h, rho, p = col["hsml"][rows], col["density"][rows], col["pressure"][rows]
    adiv, curl = np.abs(col["div_vel"][rows]), col["curl_vel"][rows]
    cs = np.sqrt(gamma * p / rho)                                                 # hydra.c:379
    tg = dict(pos=task.pos[rows], vel=vel[rows], hsml=h, mass=task.mass[rows], density=rho, pressure=p,
              dhsml_factor=col["dhsml_factor"][rows], f1=adiv / (adiv + curl + 0.0001 * cs / h / fac_mu))   # hydra.c:380-382
    if timestep is not None:
        tg["timestep"] = np.ascontiguousarray(timestep, dtype=np.int32)[rows]
    return tg


def hydro_over(tasks, vel, cols, *, art_bulk_visc_const, timestep=None, timebase_interval=0.0, gamma=5.0 / 3, viscosity_limiter=True,
               comoving=None, export=hydro_export):
    """hydro_force() of the reference over the engines of `tasks`, one round.  vel: SphP[].VelPred [n,3] per task; cols: per task
    a dict of hsml, density, pressure, dhsml_factor, div_vel, curl_vel [n] (every type-0 row is a source); timestep: None or one
    int32 [n] per task.  The sums of the engines are added, max_signal_vel by maximum, then hydra.c:320 is applied.  Returns one
    dict per task: hydro_accel [n,3], dt_entropy, max_signal_vel (rows that are no targets: 0)."""
    vel = [np.ascontiguousarray(v, dtype=np.float64) for v in vel]
    box = tasks[0].box
    hubble_a2, fac_mu = (comoving[0], comoving[1]) if comoving is not None else (1.0, 1.0)
    bounds = [t.gas_bounds(cols[a]["hsml"]) for a, t in enumerate(tasks)]
    kw = dict(art_bulk_visc_const=art_bulk_visc_const, timebase_interval=timebase_interval, gamma=gamma, viscosity_limiter=viscosity_limiter,
              comoving=comoving)

    def sums_on(b, tg):
        c = cols[b]
        return tasks[b].engine.sph_hydro_sums(vel[b], c["hsml"], c["density"], c["pressure"], c["dhsml_factor"], c["div_vel"], c["curl_vel"], tg,
                                              timestep=None if timestep is None else timestep[b], **kw)

    res = []
    for a, t in enumerate(tasks):
        n = len(t.pos)
        r = {"hydro_accel": np.zeros((n, 3)), "dt_entropy": np.zeros(n), "max_signal_vel": np.zeros(n)}
        res.append(r)
        rows = t.targets()
        if not len(rows):
            continue
        tg = hydro_targets(t, vel[a], cols[a], rows, None if timestep is None else timestep[a], gamma, fac_mu)
        sums = sums_on(a, tg)                                                     # hydro_evaluate(i, 0)
        mask = export(tg["pos"], tg["hsml"], bounds, box)
        for b in range(len(tasks)):
            sel = np.nonzero(mask[:, b])[0] if b != a else ()
            if len(sel):                                                          # hydro_evaluate(j, 1) on task b
                part = sums_on(b, {k: v[sel] for k, v in tg.items()})
                sums[sel, :4] += part[:, :4]
                sums[sel, 4] = np.maximum(sums[sel, 4], part[:, 4])
        r["hydro_accel"][rows] = sums[:, :3]
        r["dt_entropy"][rows] = sums[:, 3] * ((gamma - 1) / (hubble_a2 * np.power(tg["density"], gamma - 1)))   # hydra.c:320
        r["max_signal_vel"][rows] = sums[:, 4]
    return res
