// api_tempcontrol.hip — the C ABI of libls1hip (include/ls1hip.h), part 8: region-wise temperature control on the device (the
// reference's thermostats/TemperatureControl.{h,cpp}, method VelocityScaling, as Simulation.cpp:1137-1140 drives it).
#include "api_internal.hpp"

// d_tc, in 64-bit words: sums[4 cap] | last[4 cap] | fac[4 cap] | acc[2 TC_MAXREG]
static void tc_pointers(ls1hip_ctx* c) {
	c->tc.sums = c->d_tc;
	c->tc.last = c->d_tc + 4 * c->tc_cap;
	c->tc.fac = reinterpret_cast<double*>(c->d_tc + 8 * c->tc_cap);
	c->tc.acc = reinterpret_cast<double*>(c->d_tc + 12 * c->tc_cap);
}

static void tc_free(ls1hip_ctx* c) {
	dfree(c->d_tc);
	c->tc_cap = 0;
	c->tc = TcParams{};
	c->tc_start = c->tc_frequency = c->tc_stop = 0;
	for (auto& k : c->tc_configs) k = 0;
}

void tempcontrol_destroy(ls1hip_ctx* c) { tc_free(c); }

// TemperatureControl::readXML, control/* (TemperatureControl.cpp:579-586)
extern "C" int ls1hip_tempcontrol_config(ls1hip_ctx* c, unsigned long start, unsigned long frequency, unsigned long stop) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	if (frequency == 0) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		tc_free(c);
		return LS1HIP_OK;
	}
	REQUIRE(c, !c->thermostat_on, "the device thermostat is on: temperature control and ls1hip_set_thermostat exclude each other");
	c->tc_start = start;
	c->tc_frequency = frequency;
	c->tc_stop = stop;
	return LS1HIP_OK;
}

// ControlRegionT::readXML + VelocityScalingInit (TemperatureControl.cpp:90-236) and AddRegion (:636)
extern "C" int ls1hip_tempcontrol_region(ls1hip_ctx* c, const double lc[3], const double uc[3], double target_T, int component, unsigned numslabs,
										 double exponent, unsigned direction_mask) {
	if (!c || !lc || !uc) return LS1HIP_EINVAL;
	REQUIRE(c, c->tc_frequency > 0, "temperature control is not configured (ls1hip_tempcontrol_config)");
	REQUIRE(c, c->have_comp && c->have_domain, "ls1hip_tempcontrol_region needs the components and the domain (ls1hip_set_components, ls1hip_set_domain)");
	REQUIRE(c, c->tc.nreg < TC_MAXREG, "at most %d control regions", TC_MAXREG);
	REQUIRE(c, numslabs >= 1, "need at least one slab (settings/numslabs)");
	REQUIRE(c, direction_mask >= 1 && direction_mask <= 7, "direction_mask must be a combination of LS1HIP_TC_X | LS1HIP_TC_Y | LS1HIP_TC_Z, got %u", direction_mask);
	REQUIRE(c, component >= 0 && component <= c->h_ct.ncomp, "component must be 0 (all) or a 1-based component id up to %d, got %d", c->h_ct.ncomp, component);
	REQUIRE(c, uc[0] > lc[0] && uc[1] > lc[1] && uc[2] > lc[2], "empty region");
	REQUIRE(c, (double)c->tc.total + (double)numslabs < 536870912., "too many slabs for the 32-bit word index of the tables");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	const size_t total = (size_t)c->tc.total + numslabs;
	if (total > c->tc_cap) {
		dfree(c->d_tc);
		c->tc_cap = 0;
		const size_t cap = std::max<size_t>(total, 64);
		int rc = dalloc(c, &c->d_tc, 12 * cap + 2 * TC_MAXREG);
		if (rc) return rc;
		c->tc_cap = cap;
	}
	TcRegion& R = c->tc.reg[c->tc.nreg];
	for (int d = 0; d < 3; ++d) {
		R.lc[d] = lc[d];
		R.uc[d] = uc[d];
		R.dir[d] = (direction_mask >> d) & 1u;
	}
	R.ndir = R.dir[0] + R.dir[1] + R.dir[2];
	R.slabs = numslabs;
	R.off = c->tc.total;
	R.width = (uc[1] - lc[1]) / ((double)(numslabs));  // TemperatureControl.cpp:199
	R.target_T = target_T;
	R.exponent = exponent;
	R.comp = component;
	c->tc.nreg++;
	c->tc.total = (uint32_t)total;
	c->tc.ncomp = c->h_ct.ncomp;
	for (int d = 0; d < 3; ++d) c->tc.len[d] = c->global_len[d];
	for (auto& k : c->tc_configs) k = 0;
	tc_pointers(c);
	// every region starts again from the state before its first measurement: factors 1 with count 0
	launch_tc_init(c->tc, c->stream);
	HIPCHK(c, hipGetLastError());
	return c->tc.nreg;
}

// _dTargetTemperature of one region (the ramp of TemperatureControl.cpp:266-277 stays on the host)
extern "C" int ls1hip_tempcontrol_target(ls1hip_ctx* c, int region, double target_T) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, region >= 1 && region <= c->tc.nreg, "no region %d (%d configured)", region, c->tc.nreg);
	c->tc.reg[region - 1].target_T = target_T;
	return LS1HIP_OK;
}

static int tc_check_state(ls1hip_ctx* c) {
	REQUIRE(c, c->tc_frequency > 0 && c->tc.nreg > 0 && c->d_tc, "temperature control is not configured (ls1hip_tempcontrol_config, ls1hip_tempcontrol_region)");
	REQUIRE(c, !c->thermostat_on, "the device thermostat is on: temperature control and ls1hip_set_thermostat exclude each other");
	REQUIRE(c, c->cap_real, "no molecules uploaded");
	REQUIRE(c, !c->fused_split && !c->inner_in_flight, "a split force pass is in flight");
	REQUIRE(c, !c->half_advanced && c->pos_x != c->frc.Fx,
			"the state was advanced by a fused force + integration pass (temperature control needs full-step velocities: call after the post-force kick)");
	REQUIRE(c, c->tc.ncomp == c->h_ct.ncomp, "the component set changed since ls1hip_tempcontrol_region");
	return LS1HIP_OK;
}

TcParams tempcontrol_params(ls1hip_ctx* c) {
	const MolSoA& m = c->mol[c->cur];
	TcParams P = c->tc;
	const Pos3 r = cur_pos(c);
	P.x = r.x; P.y = r.y; P.z = r.z;
	P.vx = m.vx; P.vy = m.vy; P.vz = m.vz;
	P.q0 = m.q0; P.q1 = m.q1; P.q2 = m.q2; P.q3 = m.q3;
	P.Dx = m.Dx; P.Dy = m.Dy; P.Dz = m.Dz;
	P.cid = m.cid;
	P.ct = c->d_ct;
	P.cnt = c->d_cnt;
	return P;
}

bool tempcontrol_is_control_step(const ls1hip_ctx* c, unsigned long simstep) {
	return c->tc_frequency > 0 && c->tc.nreg > 0 && simstep % c->tc_frequency == 0;  // TemperatureControl.cpp:639, 645, 651
}

static int tc_measure(ls1hip_ctx* c) {
	TimedScope ts(c, c->t_tc_measure);
	launch_tc_measure(tempcontrol_params(c), c->h_ct.has_rot != 0, (uint32_t)c->n_real, c->stream);
	HIPCHK(c, hipGetLastError());
	return LS1HIP_OK;
}
static int tc_betas(ls1hip_ctx* c) {
	TimedScope ts(c, c->t_tc_betas);
	launch_tc_betas(c->tc, c->stream);
	HIPCHK(c, hipGetLastError());
	for (int r = 0; r < c->tc.nreg; ++r) c->tc_configs[r]++;  // _numSampledConfigs (TemperatureControl.cpp:305)
	return LS1HIP_OK;
}

// TemperatureControl::VelocityScalingPreparation (TemperatureControl.cpp:716-736) on a control step
int tempcontrol_measure_impl(ls1hip_ctx* c, unsigned long simstep) {
	if (!(c->tc_start <= simstep && c->tc_stop > simstep)) return LS1HIP_OK;  // the betas of the last measurement stay
	int rc = tc_measure(c);
	return rc ? rc : tc_betas(c);
}

int tempcontrol_apply_impl(ls1hip_ctx* c) {
	// a factor 2 - 1 / beta may exceed 1: the per-brick drift-speed bounds a list force pass left no longer bound the coming drift
	// (ls1hip_kick clears them for the same reason); the global displacement bound then decides alone
	c->vl_top2_pending = false;
	TimedScope ts(c, c->t_tc_apply);
	launch_tc_apply(tempcontrol_params(c), c->h_ct.has_rot != 0, (uint32_t)c->n_real, c->stream);
	HIPCHK(c, hipGetLastError());
	return LS1HIP_OK;
}

// TemperatureControl::DoLoopsOverMolecules (TemperatureControl.cpp:685-707)
extern "C" int ls1hip_temperature_control(ls1hip_ctx* c, unsigned long simstep) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	int rc = tc_check_state(c);
	if (rc || !tempcontrol_is_control_step(c, simstep)) return rc;
	if ((rc = tempcontrol_measure_impl(c, simstep))) return rc;
	return tempcontrol_apply_impl(c);
}

// the molecule loop of VelocityScalingPreparation (TemperatureControl.cpp:725-728): LOCAL sums, added to what the table holds
extern "C" int ls1hip_tempcontrol_measure(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	int rc = tc_check_state(c);
	return rc ? rc : tc_measure(c);
}

// the buffer of the all-reduce of ControlRegionT::CalcGlobalValues (TemperatureControl.cpp:240-264)
extern "C" int ls1hip_tempcontrol_sums_read(ls1hip_ctx* c, size_t cap_slabs, void* sums) {
	if (!c || !sums) return LS1HIP_EINVAL;
	REQUIRE(c, c->tc.nreg > 0 && c->d_tc, "temperature control is not configured");
	REQUIRE(c, cap_slabs >= c->tc.total, "buffer too small: %zu < %u slabs", cap_slabs, c->tc.total);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(sums, c->tc.sums, (size_t)c->tc.total * 32, hipMemcpyDeviceToHost));
	return LS1HIP_OK;
}
extern "C" int ls1hip_tempcontrol_sums_write(ls1hip_ctx* c, size_t nslabs, const void* sums) {
	if (!c || !sums) return LS1HIP_EINVAL;
	REQUIRE(c, c->tc.nreg > 0 && c->d_tc, "temperature control is not configured");
	REQUIRE(c, nslabs == c->tc.total, "expected the sums of %u slabs, got %zu", c->tc.total, nslabs);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(c->tc.sums, sums, (size_t)c->tc.total * 32, hipMemcpyHostToDevice));
	return LS1HIP_OK;
}

// ControlRegionT::CalcGlobalValues after the all-reduce (TemperatureControl.cpp:279-305)
extern "C" int ls1hip_tempcontrol_betas(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->tc.nreg > 0 && c->d_tc, "temperature control is not configured");
	HIPCHK(c, hipSetDevice(c->device));
	return tc_betas(c);
}

// the molecule loop of DoLoopsOverMolecules (TemperatureControl.cpp:700-703) with the factors of the last measurement
extern "C" int ls1hip_tempcontrol_apply(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	int rc = tc_check_state(c);
	return rc ? rc : tempcontrol_apply_impl(c);
}

extern "C" int ls1hip_tempcontrol_apply_kick_drift(ls1hip_ctx* c, double dt) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	int rc = tc_check_state(c);
	return rc ? rc : tempcontrol_kick_drift_impl(c, dt);
}

// _globalThermVars of one region, _dBetaTransSumGlobal / _dBetaRotSumGlobal / _numSampledConfigs (what WriteBetaLogfile reads,
// TemperatureControl.cpp:455-488; reset: its last three lines)
extern "C" int ls1hip_tempcontrol_read(ls1hip_ctx* c, int region, size_t cap_slabs, uint64_t* n, uint64_t* rot_dof, double* ekin_trans,
									   double* ekin_rot, double* beta_trans, double* beta_rot, double* beta_sums2, uint64_t* configs, int reset) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->tc.nreg > 0 && c->d_tc, "temperature control is not configured");
	REQUIRE(c, region >= 1 && region <= c->tc.nreg, "no region %d (%d configured)", region, c->tc.nreg);
	const TcRegion& R = c->tc.reg[region - 1];
	const bool slabs = n || rot_dof || ekin_trans || ekin_rot || beta_trans || beta_rot;
	REQUIRE(c, !slabs || cap_slabs >= R.slabs, "buffers too small: %zu < %u slabs", cap_slabs, R.slabs);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (slabs) {
		std::vector<unsigned long long> h(4 * (size_t)R.slabs);
		std::vector<double> f(4 * (size_t)R.slabs);
		HIPCHK(c, hipMemcpy(h.data(), c->tc.last + 4 * (size_t)R.off, h.size() * 8, hipMemcpyDeviceToHost));
		HIPCHK(c, hipMemcpy(f.data(), c->tc.fac + 4 * (size_t)R.off, f.size() * 8, hipMemcpyDeviceToHost));
		for (uint32_t s = 0; s < R.slabs; ++s) {
			double er, et;
			memcpy(&er, &h[4 * s + TC_EKIN_ROT], 8);
			memcpy(&et, &h[4 * s + TC_EKIN_TRANS], 8);
			if (n) n[s] = h[4 * s + TC_N];
			if (rot_dof) rot_dof[s] = h[4 * s + TC_ROTDOF];
			if (ekin_trans) ekin_trans[s] = et;
			if (ekin_rot) ekin_rot[s] = er;
			if (beta_trans) beta_trans[s] = f[4 * s + TC_BETA_TRANS];
			if (beta_rot) beta_rot[s] = f[4 * s + TC_BETA_ROT];
		}
	}
	if (beta_sums2) HIPCHK(c, hipMemcpy(beta_sums2, c->tc.acc + 2 * (region - 1), 16, hipMemcpyDeviceToHost));
	if (configs) *configs = c->tc_configs[region - 1];
	if (reset) {
		launch_tc_clear_acc(c->tc, region - 1, c->stream);
		HIPCHK(c, hipGetLastError());
		c->tc_configs[region - 1] = 0;
	}
	return LS1HIP_OK;
}

extern "C" int ls1hip_tempcontrol_layout(const ls1hip_ctx* c, int* regions, uint32_t* slabs8, size_t* lds_slabs, size_t* apply_lds_slabs) {
	if (!c) return LS1HIP_EINVAL;
	if (regions) *regions = c->tc.nreg;
	if (slabs8)
		for (int r = 0; r < TC_MAXREG; ++r) slabs8[r] = r < c->tc.nreg ? c->tc.reg[r].slabs : 0;
	if (lds_slabs) *lds_slabs = tempcontrol_lds_slabs();
	if (apply_lds_slabs) *apply_lds_slabs = tempcontrol_apply_lds_slabs();
	return LS1HIP_OK;
}
