// api_profile.hip — the C ABI of libls1hip (include/ls1hip.h), part 5: spatial profiles sampled on the device (the reference's
// SpatialProfile plugin: plugins/SpatialProfile.{h,cpp}, plugins/profiles/*).
#include "api_internal.hpp"

constexpr unsigned PROF_ALL_QUANT = LS1HIP_PROF_VELOCITY | LS1HIP_PROF_VELOCITY3D | LS1HIP_PROF_TEMPERATURE | LS1HIP_PROF_VIRIAL;

// words per bin of a quantity mask: n | dof, ekin | vabs | v3[3] | vi3[3]
static size_t prof_words_per_bin(unsigned q) {
	return 1 + ((q & LS1HIP_PROF_TEMPERATURE) ? 2 : 0) + ((q & LS1HIP_PROF_VELOCITY) ? 1 : 0) + ((q & LS1HIP_PROF_VELOCITY3D) ? 3 : 0) +
		   ((q & LS1HIP_PROF_VIRIAL) ? 3 : 0);
}

static void prof_free(ls1hip_ctx* c) {
	dfree(c->d_prof);
	c->prof_bins = c->prof_words = 0;
	c->prof_units[0] = c->prof_units[1] = c->prof_units[2] = 0;
	c->prof_quant = 0;
	c->prof_comp = -1;
	c->prof_samples = 0;
}

void profile_destroy(ls1hip_ctx* c) {
	prof_free(c);
	timer_free(c->t_profile);
}

// the table layout for the current configuration (ProfParams: offsets in words)
static void prof_layout(const ls1hip_ctx* c, ProfParams& P) {
	const uint32_t b = (uint32_t)c->prof_bins;
	const unsigned q = c->prof_quant;
	uint32_t at = b;
	P.off_dof = P.off_ekin = P.off_vabs = P.off_v3 = P.off_vi = 0;
	if (q & LS1HIP_PROF_TEMPERATURE) {
		P.off_dof = at;
		at += b;
	}
	P.u64_words = at;
	if (q & LS1HIP_PROF_TEMPERATURE) {
		P.off_ekin = at;
		at += b;
	}
	if (q & LS1HIP_PROF_VELOCITY) {
		P.off_vabs = at;
		at += b;
	}
	if (q & LS1HIP_PROF_VELOCITY3D) {
		P.off_v3 = at;
		at += 3 * b;
	}
	if (q & LS1HIP_PROF_VIRIAL) {
		P.off_vi = at;
		at += 3 * b;
	}
	P.bins = b;
	P.words = at;
}

extern "C" int ls1hip_profile_config(ls1hip_ctx* c, int mode, const uint32_t units[3], unsigned quantities, int component) {
	if (!c || !units) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	if (units[0] == 0 && units[1] == 0 && units[2] == 0) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		prof_free(c);
		return LS1HIP_OK;
	}
	REQUIRE(c, c->have_comp && c->have_domain, "ls1hip_profile_config needs the components and the domain (ls1hip_set_components, ls1hip_set_domain)");
	REQUIRE(c, mode == LS1HIP_PROF_CARTESIAN || mode == LS1HIP_PROF_CYLINDER, "mode must be LS1HIP_PROF_CARTESIAN or LS1HIP_PROF_CYLINDER, got %d", mode);
	REQUIRE(c, units[0] && units[1] && units[2], "every unit count must be > 0 (all three 0 switch the sampling off), got %u %u %u", units[0],
			units[1], units[2]);
	REQUIRE(c, (quantities & ~PROF_ALL_QUANT) == 0, "unknown quantity bit in 0x%x", quantities);
	REQUIRE(c, component >= -1 && component < c->h_ct.ncomp, "component must be -1 (all) or a component id below %d, got %d", c->h_ct.ncomp, component);
	const double binsd = (double)units[0] * (double)units[1] * (double)units[2];
	const size_t wpb = prof_words_per_bin(quantities);
	REQUIRE(c, binsd * (double)wpb < 2147483647., "a table of %.0f bins x %zu words exceeds the 32-bit word index", binsd, wpb);
	const size_t bins = (size_t)units[0] * units[1] * units[2];
	HIPCHK(c, hipStreamSynchronize(c->stream));
	prof_free(c);
	int rc = dalloc(c, &c->d_prof, bins * wpb);
	if (rc) return rc;
	HIPCHK(c, hipMemsetAsync(c->d_prof, 0, bins * wpb * sizeof(unsigned long long), c->stream));
	c->prof_mode = mode;
	for (int d = 0; d < 3; ++d) c->prof_units[d] = units[d];
	c->prof_quant = quantities;
	c->prof_comp = component;
	c->prof_bins = bins;
	c->prof_words = bins * wpb;
	return LS1HIP_OK;
}

extern "C" int ls1hip_profile_layout(const ls1hip_ctx* c, size_t* bins, unsigned* quantities) {
	if (!c) return LS1HIP_EINVAL;
	if (bins) *bins = c->prof_bins;
	if (quantities) *quantities = c->prof_quant;
	return LS1HIP_OK;
}

int profile_sample_impl(ls1hip_ctx* c, bool scaled) {
	REQUIRE(c, c->prof_bins > 0 && c->d_prof, "profile sampling is not configured (ls1hip_profile_config)");
	REQUIRE(c, c->cap_real, "no molecules uploaded");
	REQUIRE(c, !c->fused_split && !c->inner_in_flight, "a split force pass is in flight");
	// after a fused force + integration pass the velocities are half a step ahead and (per-step loop) the positions are parked
	// in the force arrays: not the state SpatialProfile::endStep sees
	REQUIRE(c, !c->half_advanced && c->pos_x != c->frc.Fx,
			"the state was advanced by a fused force + integration pass (sample after an unfused force pass and its kick)");
	const unsigned q = c->prof_quant;
	REQUIRE(c, !(q & LS1HIP_PROF_VIRIAL) || (c->opt_vi && c->forces_valid),
			"the virial profile needs per-molecule virials: option compute_vi=1 and valid forces (ls1hip_forces)");
	REQUIRE(c, c->prof_comp < c->h_ct.ncomp, "the component set changed since ls1hip_profile_config");
	const MolSoA& m = c->mol[c->cur];
	ProfParams P;
	memset(&P, 0, sizeof(P));
	prof_layout(c, P);
	REQUIRE(c, (size_t)P.words == c->prof_words, "profile table layout mismatch");
	P.mode = c->prof_mode;
	P.quant = q;
	P.comp = c->prof_comp;
	P.ncomp = c->h_ct.ncomp;
	P.scale = scaled ? 1 : 0;
	for (int d = 0; d < 3; ++d) {
		P.units[d] = c->prof_units[d];
		P.len[d] = c->global_len[d];
	}
	if (P.mode == LS1HIP_PROF_CYLINDER) {
		// SpatialProfile::init, cylinder branch (SpatialProfile.cpp:163-176, 210-212)
		double minXZ = c->global_len[0];
		if (c->global_len[2] < minXZ) minXZ = c->global_len[2];
		const double R2max = .24 * minXZ * minXZ;
		P.inv[0] = P.units[0] / (R2max);
		P.inv[1] = P.units[1] / (c->global_len[1]);
		P.inv[2] = P.units[2] / (2 * M_PI);
		P.centre[0] = 0.5 * c->global_len[0];
		P.centre[1] = 0;
		P.centre[2] = 0.5 * c->global_len[2];
	} else {
		for (int d = 0; d < 3; ++d) P.inv[d] = P.units[d] / c->global_len[d];  // SpatialProfile.cpp:181-183
	}
	P.x = c->pos_x ? c->pos_x : m.x; P.y = c->pos_x ? c->pos_y : m.y; P.z = c->pos_x ? c->pos_z : m.z;
	P.vx = m.vx; P.vy = m.vy; P.vz = m.vz;
	P.q0 = m.q0; P.q1 = m.q1; P.q2 = m.q2; P.q3 = m.q3;
	P.Dx = m.Dx; P.Dy = m.Dy; P.Dz = m.Dz;
	P.Vix = c->frc.Vix; P.Viy = c->frc.Viy; P.Viz = c->frc.Viz;
	P.cid = m.cid;
	P.ct = c->d_ct;
	P.cnt = c->d_cnt;
	P.tab = c->d_prof;
	{
		TimedScope ts(c, c->t_profile);
		launch_profile(P, c->h_ct.has_rot != 0, (uint32_t)c->n_real, c->stream);
	}
	HIPCHK(c, hipGetLastError());
	c->prof_samples++;  // _accumulatedDatasets (SpatialProfile.cpp:282)
	return LS1HIP_OK;
}

extern "C" int ls1hip_profile_sample(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	return profile_sample_impl(c, false);
}

extern "C" int ls1hip_profile_read(ls1hip_ctx* c, size_t cap_bins, uint64_t* n, uint64_t* dof, double* ekin, double* vabs, double* v3,
								   double* vi3, uint64_t* samples) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->prof_bins > 0 && c->d_prof, "profile sampling is not configured (ls1hip_profile_config)");
	REQUIRE(c, cap_bins >= c->prof_bins || !(n || dof || ekin || vabs || v3 || vi3), "profile buffers too small: %zu < %zu bins", cap_bins,
			c->prof_bins);
	const unsigned q = c->prof_quant;
	REQUIRE(c, (!dof && !ekin) || (q & LS1HIP_PROF_TEMPERATURE), "dof / ekin are not sampled (LS1HIP_PROF_TEMPERATURE)");
	REQUIRE(c, !vabs || (q & LS1HIP_PROF_VELOCITY), "vabs is not sampled (LS1HIP_PROF_VELOCITY)");
	REQUIRE(c, !v3 || (q & LS1HIP_PROF_VELOCITY3D), "v3 is not sampled (LS1HIP_PROF_VELOCITY3D)");
	REQUIRE(c, !vi3 || (q & LS1HIP_PROF_VIRIAL), "vi3 is not sampled (LS1HIP_PROF_VIRIAL)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	ProfParams P;
	memset(&P, 0, sizeof(P));
	prof_layout(c, P);
	const size_t b = c->prof_bins;
	if (n) HIPCHK(c, hipMemcpy(n, c->d_prof, b * 8, hipMemcpyDeviceToHost));
	if (dof) HIPCHK(c, hipMemcpy(dof, c->d_prof + P.off_dof, b * 8, hipMemcpyDeviceToHost));
	if (ekin) HIPCHK(c, hipMemcpy(ekin, c->d_prof + P.off_ekin, b * 8, hipMemcpyDeviceToHost));
	if (vabs) HIPCHK(c, hipMemcpy(vabs, c->d_prof + P.off_vabs, b * 8, hipMemcpyDeviceToHost));
	if (v3) HIPCHK(c, hipMemcpy(v3, c->d_prof + P.off_v3, 3 * b * 8, hipMemcpyDeviceToHost));
	if (vi3) HIPCHK(c, hipMemcpy(vi3, c->d_prof + P.off_vi, 3 * b * 8, hipMemcpyDeviceToHost));
	if (samples) *samples = c->prof_samples;
	return LS1HIP_OK;
}

extern "C" int ls1hip_profile_reset(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->prof_bins > 0 && c->d_prof, "profile sampling is not configured (ls1hip_profile_config)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemsetAsync(c->d_prof, 0, c->prof_words * sizeof(unsigned long long), c->stream));
	c->prof_samples = 0;
	return LS1HIP_OK;
}
