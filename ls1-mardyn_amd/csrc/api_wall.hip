// api_wall.hip — the C ABI of libls1hip (include/ls1hip.h), part 10: the external walls (the reference's plugins/WallPotential.{h,cpp}
// and plugins/Mirror.{h,cpp}), kernel in kernels_wall.hip.
#include "api_internal.hpp"

static bool any_mirror(const ls1hip_ctx* c) {
	for (const WallMirror& m : c->wl.mir)
		if (m.type != WL_MT_OFF) return true;
	return false;
}
bool wall_active(const ls1hip_ctx* c) { return c->wl.potential != WL_OFF || any_mirror(c); }

void wall_destroy(ls1hip_ctx* c) {
	dfree(c->d_wl_comp);
	dfree(c->d_wl_partials);
	dfree(c->d_wl_out);
	dfree(c->d_wl_log);
	c->wl_partials_cap = 0;
	c->wl_log_steps = 0;
	c->wl = WallParams{};
}

// the buffers a configured wall or mirror needs (kept until the context goes)
static int wall_buffers(ls1hip_ctx* c) {
	if (c->d_wl_comp) return LS1HIP_OK;
	int rc;
	if ((rc = dalloc(c, &c->d_wl_comp, MAXC)) || (rc = dalloc(c, &c->d_wl_out, MAXC)) || (rc = dalloc(c, &c->d_wl_log, STEPLOG_ROWS * MAXC))) {
		wall_destroy(c);
		return rc;
	}
	HIPCHK(c, hipMemset(c->d_wl_comp, 0, MAXC * sizeof(WallComp)));
	HIPCHK(c, hipMemset(c->d_wl_out, 0, MAXC * sizeof(double)));
	return LS1HIP_OK;
}

// WallPotential::readXML, initializeLJ93 (WallPotential.cpp:105-134), initializeLJ1043 (:147-187)
extern "C" int ls1hip_wall_config(ls1hip_ctx* c, int potential, double density, double sigma, double epsilon, double yoff, double ycut,
								  double width, double delta, int ncomp, const int* consider, const double* xi, const double* eta) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, potential == WL_OFF || potential == WL_93 || potential == WL_104, "potential must be 0 (off), 93 or 104, got %d", potential);
	HIPCHK(c, hipSetDevice(c->device));
	if (potential == WL_OFF) {
		if (c->wl.potential != WL_OFF) HIPCHK(c, hipStreamSynchronize(c->stream));
		c->wl.potential = WL_OFF;
		return LS1HIP_OK;
	}
	REQUIRE(c, c->have_comp && c->have_domain, "ls1hip_wall_config needs the components and the domain (ls1hip_set_components, ls1hip_set_domain)");
	const CompTable& ct = c->h_ct;
	REQUIRE(c, ncomp == ct.ncomp, "%d components given, the model has %d", ncomp, ct.ncomp);
	REQUIRE(c, xi && eta, "xi and eta are required");
	REQUIRE(c, ycut > 0., "ycut must be > 0, got %g", ycut);
	REQUIRE(c, width >= 0., "width must be >= 0, got %g", width);
	REQUIRE(c, potential != WL_104 || delta > 0., "the 10-4-3 wall needs delta > 0, got %g", delta);
	WallComp W[MAXC] = {};
	double d_max = 0.;
	for (int k = 0; k < ncomp; ++k) {
		W[k].consider = consider ? consider[k] != 0 : 1;
		if (!W[k].consider) continue;
		REQUIRE(c, ct.nlj[k] > 0, "component %d is considered by the wall but has no LJ centre", k + 1);
		W[k].centre = ct.nlj[k] == 1;
		for (int s = 0; s < ct.nlj[k]; ++s) {
			const double* d = ct.ljpos[ct.olj[k] + s];
			const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
			if (len != 0.) W[k].centre = 0;
			d_max = std::max(d_max, len);
		}
		const int g = ct.olj[k] * ct.ncenters + ct.olj[k];  // LJ centre 0 of the component with itself
		const double eps_i = ct.eps24[g] / 24, sig_i = sqrt(ct.sig2[g]);
		const double eps_wi = xi[k] * sqrt(epsilon * eps_i), sig_wi = 0.5 * eta[k] * (sigma + sig_i);
		const double sig2_wi = sig_wi * sig_wi, sig3_wi = sig_wi * sig_wi * sig_wi;
		if (potential == WL_93) {  // :120-133
			const double sig9_sf = sig3_wi * sig3_wi * sig3_wi;
			const double y = ycut, y3 = y * y * y, y9 = y3 * y3 * y3;
			W[k].pref = 4.0 * M_PI * density * eps_wi * sig3_wi;
			W[k].a = sig3_wi;
			W[k].b = sig9_sf;
			W[k].ushift = 4.0 / 3.0 * M_PI * density * eps_wi * sig3_wi * (sig9_sf / 15.0 / y9 - sig3_wi / 2.0 / y3);
		} else {  // :166-185; DEVIATION: 2. / 5. where the reference's integer 2 / 5 is 0
			const double sig10_sf = sig3_wi * sig3_wi * sig3_wi * sig_wi, sig4_sf = sig2_wi * sig2_wi;
			const double y = ycut, y2 = y * y, y4 = y2 * y2, y10 = y4 * y4 * y2;
			const double bracket = y + 0.61 * delta, bracket3 = bracket * bracket * bracket;
			const double sig5_wi = sig4_sf * sig_wi;  // calcTSLJ_10_4 forms its powers this way (:308-311)
			W[k].pref = 2 * M_PI * eps_wi * density * sig2_wi * delta;
			W[k].a = sig4_sf;
			W[k].b = sig5_wi * sig5_wi;
			W[k].ushift = W[k].pref * ((2. / 5.) * (sig10_sf / y10) - sig4_sf / y4 - sig4_sf / (3 * delta * bracket3));
		}
	}
	int rc = wall_buffers(c);
	if (rc) return rc;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(c->d_wl_comp, W, sizeof(W), hipMemcpyHostToDevice));
	WallParams& P = c->wl;
	P.potential = potential;
	P.ncomp = ncomp;
	P.yoff = yoff;
	P.whalf = width * 0.5;
	P.ycut = ycut;
	P.delta3 = 3 * delta;
	P.delta061 = 0.61 * delta;
	// centres that can own a site inside ycut; widened by a rounding margin (a rotated offset may exceed its length by a few ulp)
	const double reach = (P.whalf + ycut + d_max) * (1. + 1e-12) + 1e-12 * fabs(yoff);
	P.reach[0] = yoff - reach;
	P.reach[1] = yoff + reach;
	return LS1HIP_OK;
}

// Mirror::readXML (Mirror.cpp:53-187)
extern "C" int ls1hip_mirror_config(ls1hip_ctx* c, int slot, int type, int direction, double coord, int cid, double force_constant) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, slot >= 0 && slot < WL_MIRRORS, "mirror slot must be 0..%d, got %d", WL_MIRRORS - 1, slot);
	REQUIRE(c, !(type >= 3 && type <= 6),
			"mirror type %d is not served: 3 MT_ZERO_GRADIENT and 4 MT_NORMDISTR_MB are deprecated, 5 MT_MELAND_2004 and 6 MT_RAMPING delete "
			"molecules and draw random numbers", type);
	REQUIRE(c, type >= WL_MT_OFF && type <= WL_MT_FORCE, "mirror type must be 0 (off), 1 (reflect) or 2 (force constant), got %d", type);
	HIPCHK(c, hipSetDevice(c->device));
	if (type != WL_MT_OFF) {
		REQUIRE(c, direction == 0 || direction == 1, "mirror direction must be 0 (left |-o) or 1 (right o-|), got %d", direction);
		REQUIRE(c, c->have_comp, "ls1hip_mirror_config needs the components (ls1hip_set_components)");
		REQUIRE(c, cid >= 0 && cid <= c->h_ct.ncomp, "mirror cid must be 0 (all) or 1..%d, got %d", c->h_ct.ncomp, cid);
		int rc = wall_buffers(c);
		if (rc) return rc;
	}
	HIPCHK(c, hipStreamSynchronize(c->stream));
	c->wl.mir[slot] = WallMirror{type, direction, cid, coord, force_constant};
	return LS1HIP_OK;
}

int wall_impl(ls1hip_ctx* c, double* log) {
	REQUIRE(c, wall_active(c), "no wall and no mirror is configured (ls1hip_wall_config, ls1hip_mirror_config)");
	REQUIRE(c, c->cap_real, "no molecules uploaded");
	REQUIRE(c, !c->fused_split && !c->inner_in_flight, "a split force pass is in flight");
	REQUIRE(c, !c->half_advanced && c->pos_x != c->frc.Fx,
			"the state was advanced by a fused force + integration pass (the wall follows an unfused force pass)");
	REQUIRE(c, c->forces_valid, "the wall is added to valid forces (ls1hip_forces)");
	WallParams P = c->wl;
	REQUIRE(c, P.potential == WL_OFF || P.ncomp == c->h_ct.ncomp, "the component set changed since ls1hip_wall_config");
	// calcTSLJ_9_3 runs only where the container's lower face lies inside the cutoff (WallPotential.cpp:197); calcTSLJ_10_4 always
	if (P.potential == WL_93 && !(c->dom_min[1] < P.ycut + P.yoff)) P.potential = WL_OFF;
	P.ncomp = c->h_ct.ncomp;
	P.len_y = c->global_len[1];
	const uint32_t nb = wall_apply_blocks((uint32_t)c->n_real);
	if (nb > c->wl_partials_cap) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		dfree(c->d_wl_partials);
		int rc = dalloc(c, &c->d_wl_partials, (size_t)MAXC * nb);
		if (rc) return rc;
		c->wl_partials_cap = nb;
	}
	const MolSoA& m = c->mol[c->cur];
	P.comp = c->d_wl_comp;
	P.y = cur_pos(c).y;
	P.q0 = m.q0; P.q1 = m.q1; P.q2 = m.q2; P.q3 = m.q3;
	P.cid = m.cid;
	P.Fy = c->frc.Fy; P.Mx = c->frc.Mx; P.Mz = c->frc.Mz;
	P.vy = m.vy;
	P.ct = c->d_ct;
	P.cnt = c->d_cnt;
	P.partials = c->d_wl_partials;
	P.out = c->d_wl_out;
	P.log = log;
	TimedScope ts(c, c->t_wall);
	launch_wall_apply(P, c->h_ct.has_rot != 0, (uint32_t)c->n_real, c->stream);
	HIPCHK(c, hipGetLastError());
	return LS1HIP_OK;
}

extern "C" int ls1hip_wall_apply(ls1hip_ctx* c, double* upot_comp) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	int rc = wall_impl(c, nullptr);
	if (rc || !upot_comp) return rc;
	double h[MAXC];
	HIPCHK(c, hipMemcpyAsync(h, c->d_wl_out, sizeof(h), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	std::copy(h, h + c->h_ct.ncomp, upot_comp);
	return LS1HIP_OK;
}

extern "C" int ls1hip_wall_log(ls1hip_ctx* c, size_t cap_rows, double* rows, size_t* nrows) {
	if (!c) return LS1HIP_EINVAL;
	const size_t have = c->d_wl_log ? std::min<size_t>(c->wl_log_steps, STEPLOG_ROWS) : 0;
	if (nrows) *nrows = have;
	if (!rows || have == 0) return LS1HIP_OK;
	REQUIRE(c, cap_rows >= have, "buffer too small: %zu < %zu rows", cap_rows, have);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	std::vector<double> ring(have * MAXC);
	int rc = ring_read(c, c->d_wl_log, MAXC * sizeof(double), c->wl_log_steps, STEPLOG_ROWS, ring.data());
	if (rc) return rc;
	const int ncomp = c->h_ct.ncomp;  // the device rows hold MAXC doubles, the caller's ncomp
	for (size_t r = 0; r < have; ++r) std::copy(&ring[r * MAXC], &ring[r * MAXC] + ncomp, rows + r * ncomp);
	return LS1HIP_OK;
}
