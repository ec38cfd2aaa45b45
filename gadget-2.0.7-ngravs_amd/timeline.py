"""The reference's main loop (run.c:32-65) for ONE task on an Engine: sync point, drift, hand-over, accelerations, gas,
displacement constraint, advance -- every station a call of the library, on columns that stay where they are.

    tl = Timeline(engine, cols, par, sph=dict(des_num_ngb=..., max_num_ngb_deviation=..., art_bulk_visc_const=...))
    while tl.ti_current < abi.TIMEBASE:
        tl.step()

cols is the host's P[] and SphP[] as a dict of columns, numpy arrays or contiguous torch tensors on the device (float64; int32
for type and the two Ti columns): type, pos, vel, mass, ti_begstep, ti_endstep, grav_accel, grav_pm, old_acc, and with gas
vel_pred, hydro_accel, entropy, dt_entropy, density, hsml, pressure, div_vel, curl_vel, dhsml_factor, max_signal_vel.  All are
updated in place.  With device tensors no column crosses to the host: the loop reads back the scalars of the sync point and,
on full steps, the 18 displacement sums, and with time_bet_statistics the 78 sums of the energy statistics (run.c:52-59) when due.
"""
import ctypes as C
import math

import numpy as np

from . import abi

TIME_COLS = abi.TIME_COL_NAMES
GAS_COLS = ("vel_pred", "hydro_accel", "entropy", "dt_entropy", "density", "hsml", "pressure", "div_vel", "curl_vel", "dhsml_factor",
            "max_signal_vel")


def _addr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


class Timeline:
    """ti_current, time, pm_ti ([PM_Ti_begstep, PM_Ti_endstep], None without a mesh), dt_displacement, full_step and n_active
    are the reference's globals of the same names after the last step()."""

    def __init__(self, engine, cols, par, sph=None, tree_domain_update_frequency=0.0, softening=None, on_station=None,
                 time_bet_statistics=None, energy_file=None, potential=None, output=None):
        """par: abi.make_time_params(...).  sph: the keyword arguments of Engine.sph_accelerations that are not columns or times
        (des_num_ngb, max_num_ngb_deviation, art_bulk_visc_const, ...), required with gas.  tree_domain_update_frequency:
        All.TreeDomainUpdateFrequency (domain.c:66-76); 0 decomposes and builds on every step.  softening: None, or a function
        of All.Time that returns All.ForceSoftening[6] (set_softenings(), gravtree.c:468-518, for comoving runs).  on_station:
        None, or a function called as on_station(name, timeline) in front of the stations "drift" and "advance", when the particles
        have "moved", and at the "end" of a step.  The reference's start (init.c): Ti_begstep = Ti_endstep = 0 for every row, Ti_Current = 0.
        time_bet_statistics: None (no energy statistics), or All.TimeBetStatistics: whenever All.Time has passed the last
        statistics by that much (run.c:52-59), on_station("statistics", timeline) is called in front of the "advance" station,
        sys_state becomes the abi.SysState of compute_global_quantities_of_system(), and the line of energy.txt is appended to
        energy_lines and to energy_file (a path opened for append, or an object with write).  potential: None (no potentials:
        EnergyPot is 0 and no POT block), a function of the timeline that returns the P[].Potential column (of the kind of the
        columns) or None, or "device": the statistics and the snapshot station call Engine.compute_potential on the columns as
        drifted (compute_potential(), potential.c:22-345; the snapshot station hands the moved particles over and builds the tree
        first, potential.c:50-61) and potential_column is that column afterwards.
        output: None (no snapshot files; the loop is then exactly the one without this argument), or a dict: dir (All.OutputDir,
        with its separator), base (All.SnapshotFileBase), snap_format (1 or 2), rule (abi.make_output_rule: the list of output
        times, or TimeOfFirstSnapshot / TimeBetSnapshot), blocks_mask (abi.snap_mask), mass_table (All.MassTable), ids (a function
        of the timeline that returns the P[].ID column, int32, of the kind of the columns), and optionally buffer_bytes and
        hubble_param.  Whenever the next sync point has reached ti_nextoutput (run.c:206-225) the particles are moved to the
        output time, on_station("snapshot", timeline) is called and <dir><base>_%03d is written (snapshot_file_count counts them,
        snapshot_files lists them); the POT block is written when `potential` gives a column."""
        from . import lib
        self._lib = lib()
        self.eng, self.cols, self.par = engine, cols, par
        self.sph = dict(sph or {})
        self.freq = float(tree_domain_update_frequency)
        self.softening, self.on_station = softening, on_station
        self.n = int(cols["pos"].shape[0])
        self.device = hasattr(cols["pos"], "data_ptr")
        self.mesh = engine.cfg.pmgrid > 0
        self.n_gas = int((cols["type"] == 0).sum())
        if self.n_gas and not all(k in cols for k in GAS_COLS):
            raise ValueError("gas needs the columns %s" % (GAS_COLS,))
        cols["ti_begstep"][:] = 0
        cols["ti_endstep"][:] = 0
        self.ti_current, self.pm_ti = 0, [0, 0] if self.mesh else None
        self.time = par.time_begin
        self.dt_displacement, self.full_step, self.n_active = 0.0, True, 0
        self.num_forces_since_decomp = 1 + self.n * self.freq   # (begrun: the first step decomposes)
        self.have_tree = False
        self.steps = 0
        self.time_bet_statistics = None if time_bet_statistics is None else float(time_bet_statistics)
        if self.time_bet_statistics is not None:
            self.time_last_statistics = par.time_begin - self.time_bet_statistics   # init.c:94
        if isinstance(potential, str) and potential != "device":
            raise ValueError('potential: None, a function of the timeline, or "device"')
        self.potential, self.sys_state, self.energy_lines = potential, None, []
        self.potential_column = None
        self._energy_file = open(energy_file, "a") if isinstance(energy_file, (str, bytes)) or hasattr(energy_file, "__fspath__") else energy_file
        self.output = None if output is None else dict(output)
        if self.output is not None:
            unknown = set(self.output) - {"dir", "base", "snap_format", "rule", "blocks_mask", "mass_table", "ids", "buffer_bytes", "hubble_param"}
            if unknown or "rule" not in self.output or "ids" not in self.output:
                raise TypeError("output: dir, base, snap_format, rule, blocks_mask, mass_table, ids[, buffer_bytes, hubble_param]")
            from . import find_next_outputtime
            self.ti_nextoutput = find_next_outputtime(par, self.output["rule"], 0)   # begrun.c:141
            self.snapshot_file_count = 0
            self.snapshot_files = []

    def _station(self, name):
        if self.on_station:
            self.on_station(name, self)

    def _time_cols(self, names):
        return {k: self.cols[k] for k in names if k in self.cols}

    def _hand_over(self, rebuild, pos=None):
        """P[] to the engine: a new particle set in front of a decomposition, else the drifted rows of the kept tree.  pos: the
        position column to hand over instead of the caller's"""
        c = self.cols
        pos = c["pos"] if pos is None else pos
        if self.device:
            import torch
            act = (c["ti_endstep"] == self.ti_current).to(torch.uint8)
            torch.cuda.synchronize()   # the library works on a stream of its own
        else:
            act = (c["ti_endstep"] == self.ti_current).astype(np.uint8)
        p = abi.Particles()
        p.n = self.n
        p.pos, p.pos_stride = _addr(pos), 24
        p.mass, p.mass_stride = _addr(c["mass"]), 8
        p.type, p.type_stride = _addr(c["type"]), 4
        p.old_acc, p.old_acc_stride = _addr(c["old_acc"]), 8
        p.active, p.active_stride = _addr(act), 1
        if self.mesh and rebuild:
            p.grav_pm, p.grav_pm_stride = _addr(c["grav_pm"]), 24
        p.on_device = int(self.device)
        eng = self.eng
        if rebuild:
            eng.n = self.n
            eng._check(self._lib.ngravs_set_particles(eng._h, C.byref(p)), "ngravs_set_particles")
        else:
            eng._check(self._lib.ngravs_update_particles(eng._h, C.byref(p)), "ngravs_update_particles")
            eng.force_update_tree()
        if self.par.adaptive_gravsoft and self.n_gas:
            eng.set_gas_softening(c["hsml"])
        self._active = act

    def _fetch_accel(self):
        """GravAccel and OldAcc of the active rows, GravPM of all rows, into the caller's columns (gravtree.c:318-341)"""
        c, eng = self.cols, self.eng
        eng._check(self._lib.ngravs_get_accel(eng._h, _addr(c["grav_accel"]), 24, _addr(c["grav_pm"]) if self.mesh else None, 24,
                                              _addr(c["old_acc"]), 8, None, 0, int(self.device), 1), "ngravs_get_accel")

    def _potential(self, moved):
        """the P[].Potential column of a station, or None.  "device": compute_potential() of the engine; moved: the columns have
        been drifted since the engine saw them, so they are handed over and the tree is built first (potential.c:50-61) -- a
        periodic run hands over the positions mapped back onto the box, which the potential does not notice"""
        if self.potential != "device":
            return self.potential(self) if self.potential else None
        eng, c = self.eng, self.cols
        if moved:
            pos = c["pos"]
            if eng.cfg.periodic:
                box = eng.cfg.box_size
                pos = pos - box * (pos / box).floor() if self.device else pos - box * np.floor(pos / box)
                pos[pos >= box] = 0.0   # (-1e-17 + box rounds to box)
            self._hand_over(True, pos=pos)
            eng.domain_Decomposition()
            eng.force_treebuild()
            self.have_tree = True
        if self.potential_column is None:
            if self.device:
                import torch
                self.potential_column = torch.zeros(self.n, dtype=torch.float64, device=c["pos"].device)
            else:
                self.potential_column = np.zeros(self.n)
        eng.compute_potential(self.par, into=self.potential_column)
        return self.potential_column

    def _statistics(self):
        """energy_statistics() (run.c:413-433) on the columns as they are, with compute_potential() first when potential is "device" """
        from . import energy_line
        self._station("statistics")
        pot = self._potential(moved=False)
        self.sys_state = self.eng.global_quantities(self._time_cols(TIME_COLS), self.par, self.ti_current, self.pm_ti, pot)
        line = energy_line(self.sys_state, self.time)
        self.energy_lines.append(line)
        if self._energy_file is not None:
            self._energy_file.write(line)
            self._energy_file.flush()
        self.time_last_statistics += self.time_bet_statistics

    def _time_of(self, ti):
        par = self.par
        if par.comoving:
            return par.time_begin * math.exp(ti * par.timebase_interval)
        return par.time_begin + ti * par.timebase_interval

    def write_snapshot(self):
        """savepositions(All.SnapshotFileCount++) on the columns as they are, at ti_current (run.c:222; a caller writes the last
        snapshot of run.c:136 with it).  Returns the file's path."""
        import os
        o = self.output
        if o is None:
            raise ValueError("the timeline has no output=")
        self._station("snapshot")
        pot = self._potential(moved=True)
        mask = int(o.get("blocks_mask", abi.SNAP_ALWAYS))
        mask = (mask | (1 << abi.SNAP_POT)) if pot is not None else (mask & ~(1 << abi.SNAP_POT))
        path = "%s%s_%03d" % (os.fspath(o.get("dir", "")), o.get("base", "snapshot"), self.snapshot_file_count)
        self.eng.write_snapshot(path, self._time_cols(TIME_COLS), self.par, self.ti_current, pm_ti=self.pm_ti, mass_table=o.get("mass_table"),
                                ids=o["ids"](self), potential=pot, blocks_mask=mask, snap_format=o.get("snap_format", 1),
                                buffer_bytes=o.get("buffer_bytes", 0), hubble_param=o.get("hubble_param", 0.0))
        self.snapshot_file_count += 1
        self.snapshot_files.append(path)
        return path

    def step(self):
        """one pass of the main loop (run.c:36-61); returns ti_current"""
        eng, c, par = self.eng, self.cols, self.par
        # 1. find_next_sync_point_and_drift (run.c:151-234)
        ti_next, self.full_step, self.n_active = eng.next_sync_point(c["ti_endstep"], self.pm_ti[1] if self.mesh else None)
        self.num_forces_since_decomp += self.n_active
        pm_step = self.mesh and self.pm_ti[1] == ti_next
        if pm_step:   # domain.c:66-73
            self.num_forces_since_decomp = 1 + self.n * self.freq
        rebuild = not self.have_tree or self.num_forces_since_decomp > self.n * self.freq   # domain.c:76
        # 1a. the output times that the sync point has reached (run.c:206-225)
        if self.output is not None:
            from . import find_next_outputtime
            while ti_next >= self.ti_nextoutput and self.ti_nextoutput >= 0:
                eng.move_particles(self._time_cols(TIME_COLS), par, self.ti_current, self.ti_nextoutput, wrap=False)
                self.ti_current = self.ti_nextoutput
                self.time = self._time_of(self.ti_current)
                self.write_snapshot()
                self.ti_nextoutput = find_next_outputtime(par, self.output["rule"], self.ti_nextoutput + 1)
        self._station("drift")
        # 2. the drift; in front of a decomposition the particles are mapped back onto the box (domain.c:80-82)
        self.wrapped = bool(rebuild and eng.cfg.periodic)
        eng.move_particles(self._time_cols(TIME_COLS), par, self.ti_current, ti_next, wrap=rebuild)
        self.ti_previous, self.ti_current = self.ti_current, ti_next
        self._station("moved")
        if par.comoving:
            self.time = par.time_begin * math.exp(ti_next * par.timebase_interval)
        else:
            self.time = par.time_begin + ti_next * par.timebase_interval
        if self.softening:
            eng.set_softening(self.softening(self.time))
        # 3. domain_Decomposition, or the kept tree
        self._hand_over(rebuild)
        if rebuild:
            self.num_forces_since_decomp = 0
        # 4. compute_accelerations (accel.c:24-58); at the start twice, the second time with the OldAcc of the first
        eng.compute_accelerations(pm_step)
        self.have_tree = True
        self._fetch_accel()
        if self.ti_current == 0 and eng.cfg.err_tol_theta == 0:
            eng._check(self._lib.ngravs_set_old_acc(eng._h, _addr(c["old_acc"]), 8, int(self.device)), "ngravs_set_old_acc")
            eng.gravity_tree()
            self._fetch_accel()
        # 5. density, pressure and hydro forces of the active gas (accel.c:60-89)
        if self.n_gas:
            comoving = None
            if par.comoving:
                from . import hydro_factors
                comoving = hydro_factors(self.time, par.omega0, par.omega_lambda, par.hubble, par.gamma)
            out = dict(hydro_accel=c["hydro_accel"], dt_entropy_out=c["dt_entropy"], max_signal_vel=c["max_signal_vel"])
            self.sph_result = eng.sph_accelerations(
                c["vel_pred"], c["entropy"], c["hsml"], c["density"], c["pressure"], c["dhsml_factor"], c["div_vel"], c["curl_vel"],
                dt_entropy=c["dt_entropy"], ti_begstep=c["ti_begstep"], ti_endstep=c["ti_endstep"], ti_current=self.ti_current,
                timebase_interval=par.timebase_interval, gamma=par.gamma, min_gas_hsml=par.min_gas_hsml, comoving=comoving, out=out,
                **self.sph)
        # 6. the displacement constraint, on full steps (timestep.c:63-68)
        if self.full_step or self.dt_displacement == 0:
            self.disp_sums = eng.displacement_sums(c["type"], c["vel"], c["mass"])
            self.dt_displacement = eng.dt_displacement(par, self.disp_sums, self.time)
        # 7. energy_statistics, when due (run.c:52-59)
        if self.time_bet_statistics is not None and self.time - self.time_last_statistics >= self.time_bet_statistics:
            self._statistics()
        # 8. advance_and_find_timesteps
        self._station("advance")
        self.n_kicked, pm_ti = eng.advance_and_find_timesteps(self._time_cols(TIME_COLS), par, self.ti_current, self.dt_displacement,
                                                              self.pm_ti)
        if pm_step:
            self.pm_ti = pm_ti
            self.num_forces_since_decomp = 1 + self.n * self.freq   # timestep.c:77-81: the nodes were not kicked
        self.steps += 1
        self._station("end")
        return self.ti_current
