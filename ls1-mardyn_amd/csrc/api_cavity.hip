// api_cavity.hip — the C ABI of libls1hip (include/ls1hip.h), part 10: cavity detection on the device (the reference's CavityWriter
// plugin and its CavityEnsemble: io/CavityWriter.cpp, ensemble/CavityEnsemble.cpp).
#include "api_internal.hpp"

constexpr size_t CAV_SERIES = 4096;  // n_active of the last samples kept on the device (ring, like the step log)

static void cavity_free(ls1hip_ctx* c) {
	dfree(c->d_cav_flags);
	dfree(c->d_cav_counts);
	dfree(c->d_cav_series);
	memset(&c->cav, 0, sizeof(c->cav));
	c->cav_radius = 0.;
	c->cav_samples = 0;
	c->cav_last_counts = false;
}

void cavity_destroy(ls1hip_ctx* c) { cavity_free(c); }

// CavityWriter::readXML (CavityWriter.cpp:40-90) + CavityEnsemble::setSystem / setControlVolume / setSubdomain / init
// (CavityEnsemble.cpp:49-112, :135-160)
extern "C" int ls1hip_cavity_config(ls1hip_ctx* c, int nx, int ny, int nz, int max_neighbours, float radius, const double cv_min[3],
									 const double cv_max[3]) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	REQUIRE(c, c->have_comp && c->have_domain, "ls1hip_cavity_config needs the components and the domain (ls1hip_set_components, ls1hip_set_domain)");
	REQUIRE(c, max_neighbours > 0, "maxNeighbours must be > 0, got %d", max_neighbours);  // CavityWriter.cpp:41
	REQUIRE(c, radius > 0.0f && std::isfinite(radius), "radius must be > 0, got %g", (double)radius);  // :47
	// the halo shell and the cell walk guarantee every entry within r_c of a point of the subdomain, not more
	REQUIRE(c, (double)radius <= c->rc, "radius %g exceeds the cutoff r_c = %g", (double)radius, c->rc);
	REQUIRE(c, nx > 0 && ny > 0 && nz > 0, "Nx, Ny, Nz must be > 0, got %d %d %d", nx, ny, nz);  // :52-65
	REQUIRE(c, (cv_min == nullptr) == (cv_max == nullptr), "cv_min and cv_max come together (both NULL: the whole domain)");
	const uint64_t nodes = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;  // < 2^93 / overflow: checked by division
	REQUIRE(c, nodes / (uint64_t)nx / (uint64_t)ny == (uint64_t)nz && nodes <= 0xffffffffull,
			"a lattice of %d x %d x %d nodes exceeds the 2^32 - 1 node ids", nx, ny, nz);
	CavityParams P;
	memset(&P, 0, sizeof(P));
	const int N[3] = {nx, ny, nz};
	uint64_t local = 1;
	for (int d = 0; d < 3; ++d) {
		const double cb = cv_min ? cv_min[d] : 0., ct = cv_max ? cv_max[d] : c->global_len[d];
		// CavityWriter.cpp:78-90 refuses cb > ct and bounds outside the domain; cb == ct has no lattice (CavityEnsemble.cpp:97: exit 711)
		REQUIRE(c, cb < ct && cb >= 0. && ct <= c->global_len[d], "control volume [%g, %g) of dimension %d is empty or leaves the domain [0, %g]", cb, ct,
				d, c->global_len[d]);
		P.glen[d] = c->global_len[d];
		P.cb[d] = cb;
		P.h[d] = (ct - cb) / (double)N[d];  // grid_spacing, CavityEnsemble.cpp:158
		P.N[d] = (uint32_t)N[d];
		// minredco / maxredco are float members (CavityEnsemble.h), minlu / maxlu: CavityEnsemble.cpp:144-145.  The reference lets the
		// loop bounds leave [0, N) when the control volume is smaller than the subdomain; the lattice ends at the control volume here.
		const float minred = (float)((c->dom_min[d] - cb) / (ct - cb)), maxred = (float)((c->dom_max[d] - cb) / (ct - cb));
		long lo = (long)std::round((double)N[d] * minred - 0.0009756), hi = (long)std::round((double)N[d] * maxred - 0.0009756) - 1;
		lo = std::max(lo, 0L);
		hi = std::min(hi, (long)N[d] - 1);
		P.lo[d] = (uint32_t)std::min(lo, (long)N[d]);
		P.n[d] = hi >= lo ? (uint32_t)(hi - lo + 1) : 0u;
		local *= P.n[d];
	}
	const float rr = radius * radius;  // setSystem(..., float radius): the product is formed in float (:51)
	P.RR = (double)rr;
	P.max_nb = (uint32_t)max_neighbours;
	if (local) {
		cavity_tile_shape(P.n, P.h, std::sqrt(P.RR), P.tile);
		uint64_t nt = 1;
		for (int d = 0; d < 3; ++d) {
			P.nt[d] = (P.n[d] + P.tile[d] - 1) / P.tile[d];
			nt *= P.nt[d];
		}
		REQUIRE(c, nt < 0x7ffffff0ull, "%llu tiles exceed the launch grid", (unsigned long long)nt);
		P.ntiles = (uint32_t)nt;
	}
	HIPCHK(c, hipStreamSynchronize(c->stream));
	cavity_free(c);
	int rc;
	if ((rc = dalloc(c, &c->d_cav_flags, (size_t)local)) || (rc = dalloc(c, &c->d_cav_series, CAV_SERIES))) return rc;
	HIPCHK(c, hipMemsetAsync(c->d_cav_flags, 0, std::max<size_t>(local, 1), c->stream));
	HIPCHK(c, hipMemsetAsync(c->d_cav_series, 0, CAV_SERIES * sizeof(unsigned long long), c->stream));
	c->cav = P;
	c->cav_radius = (double)radius;
	for (int d = 0; d < 3; ++d) {
		c->cav_dom[d] = c->dom_min[d];
		c->cav_dom[3 + d] = c->dom_max[d];
	}
	return LS1HIP_OK;
}

static bool cavity_configured(const ls1hip_ctx* c) { return c->d_cav_flags != nullptr; }
static size_t cavity_local_nodes(const ls1hip_ctx* c) { return (size_t)c->cav.n[0] * c->cav.n[1] * c->cav.n[2]; }

// one CavityEnsemble::cavityStep (CavityEnsemble.cpp:313-330) over the current positions; any cells_in_cutoff (the cells are found
// from coordinates, not from a fixed neighbourhood)
int cavity_sample_impl(ls1hip_ctx* c) {
	REQUIRE(c, cavity_configured(c), "cavity detection is not configured (ls1hip_cavity_config)");
	REQUIRE(c, c->cap_real, "no molecules uploaded");
	if (int rc = sample_gate(c)) return rc;
	CavityParams P = c->cav;
	for (int d = 0; d < 3; ++d)
		REQUIRE(c, P.glen[d] == c->global_len[d] && c->cav_dom[d] == c->dom_min[d] && c->cav_dom[3 + d] == c->dom_max[d],
				"the domain changed since ls1hip_cavity_config");
	REQUIRE(c, (double)c->cav_radius <= c->rc, "the cutoff changed since ls1hip_cavity_config: radius %g > r_c = %g", c->cav_radius, c->rc);
	const size_t local = cavity_local_nodes(c);
	const bool counts = c->opt_cavity_counts != 0;
	if (counts && !c->d_cav_counts) {
		int rc = dalloc(c, &c->d_cav_counts, local);
		if (rc) return rc;
	}
	const Pos3 r = cur_pos(c);
	P.g = c->g;
	P.x = r.x; P.y = r.y; P.z = r.z;
	P.id = c->mol[c->cur].id;
	P.cell_begin = c->d_cell_begin; P.cell_end = c->d_cell_end;
	// the pre-filter keeps everything a node of the tile can reach (|d| <= sqrt(dd) < R, rounding far inside the 2^-40); between two
	// list builds an entry sits in the cell of its position at build time, at most `skin` away (the local rebuild criterion bounds the
	// displacement of PAIRS by skin, a single molecule may have moved by all of it)
	const double R = std::sqrt(P.RR);
	P.rfilter = R * (1. + 0x1p-40);
	P.rwalk = (R + (c->vl_on ? c->vl_skin : 0.)) * (1. + 0x1p-40);
	P.chunk = (uint32_t)cavity_chunk_max();
	if (c->opt_cavity_chunk > 0) P.chunk = (uint32_t)std::min<long>(c->opt_cavity_chunk, (long)P.chunk);
	P.flags = c->d_cav_flags;
	P.counts = counts ? c->d_cav_counts : nullptr;
	P.n_active = c->d_cav_series + c->cav_samples % CAV_SERIES;
	if (P.ntiles) {
		TimedScope ts(c, c->t_cavity);
		launch_cavity(P, c->stream);
	}
	HIPCHK(c, hipGetLastError());
	c->cav_samples++;
	c->cav_last_counts = counts;
	return LS1HIP_OK;
}

extern "C" int ls1hip_cavity_sample(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	return cavity_sample_impl(c);
}

extern "C" int ls1hip_cavity_read(ls1hip_ctx* c, uint32_t lo[3], uint32_t n[3], uint8_t* flags, uint32_t* counts, size_t cap, uint64_t* n_active) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, cavity_configured(c), "cavity detection is not configured (ls1hip_cavity_config)");
	const size_t local = cavity_local_nodes(c);
	for (int d = 0; d < 3; ++d) {
		if (lo) lo[d] = c->cav.lo[d];
		if (n) n[d] = c->cav.n[d];
	}
	REQUIRE(c, (!flags && !counts) || cap >= local, "buffer too small: %zu < %zu nodes", cap, local);
	REQUIRE(c, !counts || c->cav_last_counts, "counts were asked for, but the last sample did not run in count mode (option cavity_counts)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (flags && local) HIPCHK(c, hipMemcpy(flags, c->d_cav_flags, local, hipMemcpyDeviceToHost));
	if (counts && local) HIPCHK(c, hipMemcpy(counts, c->d_cav_counts, local * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (n_active) {
		*n_active = 0;
		if (c->cav_samples)
			HIPCHK(c, hipMemcpy(n_active, c->d_cav_series + (c->cav_samples - 1) % CAV_SERIES, sizeof(uint64_t), hipMemcpyDeviceToHost));
	}
	return LS1HIP_OK;
}

extern "C" int ls1hip_cavity_series(ls1hip_ctx* c, size_t cap, uint64_t* n_active, size_t* samples) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, cavity_configured(c), "cavity detection is not configured (ls1hip_cavity_config)");
	const size_t have = (size_t)std::min<uint64_t>(c->cav_samples, CAV_SERIES);
	if (samples) *samples = have;
	if (!n_active || have == 0) return LS1HIP_OK;
	REQUIRE(c, cap >= have, "buffer too small: %zu < %zu samples", cap, have);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return ring_read(c, c->d_cav_series, sizeof(uint64_t), c->cav_samples, CAV_SERIES, n_active);  // a ring over the sample number
}
