// api_insert.hip — the C ABI of libls1hip (include/ls1hip.h), part 7: energies of test-particle insertions and Widom sampling
// (the reference's ensemble/ChemicalPotential.cpp:451-591 with LinkedCells::getEnergy, particleContainer/LinkedCells.cpp:998-1052).
#include "api_internal.hpp"

static void widom_free(ls1hip_ctx* c) {
	dfree(c->d_widom);
	memset(&c->wd, 0, sizeof(c->wd));
	c->wd_samples = 0;
	c->wd_last = 0;
}

void insert_destroy(ls1hip_ctx* c) {
	widom_free(c);
	dfree(c->d_ins);
	c->ins_cap = 0;
}

// the state rules of the sampling passes, and the arguments every insertion launch shares
static int insert_params(ls1hip_ctx* c, InsertParams* out) {
	REQUIRE(c, c->have_comp && c->have_domain && c->cap_real, "no molecules uploaded");
	// between two builds of the neighbour lists the binning of the last build stays: a partner inside r_c of the test point now was
	// inside r_c + skin / 2 of it at build time, and the cells are at least r_c + skin long
	if (int rc = sample_gate(c)) return rc;
	InsertParams P;
	memset(&P, 0, sizeof(P));
	fill_cell_args(c, P);
	P.id = c->mol[c->cur].id;
	P.hsrc = c->d_halo_src;
	P.eps24 = c->h_ct.eps24[0]; P.sig2 = c->h_ct.sig2[0]; P.shift6 = c->h_ct.shift6[0];
	*out = P;
	return LS1HIP_OK;
}

static int insert_mode(const ls1hip_ctx* c) {
	const CompTable& t = c->h_ct;
	bool lj_only = true;
	for (int k = 0; k < t.ncomp; ++k) lj_only = lj_only && t.nc[k] + t.nd[k] + t.nq[k] == 0;
	return c->one_clj ? 0 : (lj_only ? 1 : 2);
}

static int insert_launch(ls1hip_ctx* c, const InsertParams& P) {
	{
		TimedScope ts(c, c->t_insert);
		launch_insert(P, insert_mode(c), c->h_ct.has_rot != 0, c->stream);
	}
	HIPCHK(c, hipGetLastError());
	return LS1HIP_OK;
}

extern "C" int ls1hip_insertion_energies(ls1hip_ctx* c, size_t n, const int32_t* cid, const double* r, const double* q,
										  const uint64_t* exclude_id, double* dU) {
	if (!c) return LS1HIP_EINVAL;
	if (n == 0) return LS1HIP_OK;
	REQUIRE(c, cid && r && dU, "cid, r and dU are required");
	REQUIRE(c, n < (size_t)0x7fffffff, "%zu tests exceed the 32-bit test index", n);
	HIPCHK(c, hipSetDevice(c->device));
	InsertParams P;
	int rc = insert_params(c, &P);
	if (rc) return rc;
	for (size_t k = 0; k < n; ++k) {
		REQUIRE(c, cid[k] >= 0 && cid[k] < c->h_ct.ncomp, "test %zu: component id %d out of range [0, %d)", k, (int)cid[k], c->h_ct.ncomp);
		REQUIRE(c, q || c->h_ct.rotdof[cid[k]] == 0, "test %zu: component %d rotates, q is required", k, (int)cid[k]);
		for (int d = 0; d < 3; ++d)
			REQUIRE(c, r[3 * k + d] >= c->g.bmin[d] && r[3 * k + d] < c->g.bmax[d],
					"test %zu: position %.17g outside the box [%.17g, %.17g) in dimension %d", k, r[3 * k + d], c->g.bmin[d], c->g.bmax[d], d);
	}
	// staging {r[n][3], q[n][4], dU[n], exclude_id[n], cid[n]}: grows, never shrinks
	if (n > c->ins_cap) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		dfree(c->d_ins);
		c->ins_cap = 0;
		const size_t cap = std::max<size_t>(n, 1024);
		if ((rc = dalloc(c, &c->d_ins, cap * (9 * sizeof(double) + sizeof(int32_t))))) return rc;
		c->ins_cap = cap;
	}
	const size_t cap = c->ins_cap;
	double* const d_r = (double*)c->d_ins;
	double* const d_q = d_r + 3 * cap;
	double* const d_dU = d_q + 4 * cap;
	uint64_t* const d_ex = (uint64_t*)(d_dU + cap);
	int32_t* const d_cid = (int32_t*)(d_ex + cap);
	HIPCHK(c, hipMemcpyAsync(d_r, r, n * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
	if (q) HIPCHK(c, hipMemcpyAsync(d_q, q, n * 4 * sizeof(double), hipMemcpyHostToDevice, c->stream));
	if (exclude_id) HIPCHK(c, hipMemcpyAsync(d_ex, exclude_id, n * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(c, hipMemcpyAsync(d_cid, cid, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
	P.n = (uint32_t)n;
	P.tcid = d_cid;
	P.tr = d_r;
	P.tq = q ? d_q : nullptr;
	P.excl = exclude_id ? d_ex : nullptr;
	P.dU = d_dU;
	if ((rc = insert_launch(c, P))) return rc;
	HIPCHK(c, hipMemcpyAsync(dU, d_dU, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return LS1HIP_OK;
}

extern "C" int ls1hip_widom_config(ls1hip_ctx* c, int component, uint32_t instances, double temperature, uint64_t seed, int slabs,
									const double cv_min[3], const double cv_max[3]) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	if (instances == 0) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		widom_free(c);
		return LS1HIP_OK;
	}
	REQUIRE(c, c->have_comp && c->have_domain, "ls1hip_widom_config needs the components and the domain (ls1hip_set_components, ls1hip_set_domain)");
	REQUIRE(c, component >= 0 && component < c->h_ct.ncomp, "component id %d out of range [0, %d)", component, c->h_ct.ncomp);
	REQUIRE(c, instances < 0x7fffffffu, "instances must be below 2^31, got %u", instances);
	REQUIRE(c, temperature > 0. && std::isfinite(temperature), "temperature must be > 0, got %g", temperature);
	REQUIRE(c, slabs >= 1 && slabs <= (1 << 24), "slabs must be in [1, 2^24], got %d", slabs);
	REQUIRE(c, (cv_min == nullptr) == (cv_max == nullptr), "cv_min and cv_max come together (both NULL: the whole box)");
	WidomParams W;
	memset(&W, 0, sizeof(W));
	for (int d = 0; d < 3; ++d) {
		W.lo[d] = cv_min ? cv_min[d] : c->g.bmin[d];
		W.hi[d] = cv_max ? cv_max[d] : c->g.bmax[d];
		REQUIRE(c, W.lo[d] >= c->g.bmin[d] && W.hi[d] <= c->g.bmax[d] && W.lo[d] < W.hi[d],
				"control volume [%g, %g) of dimension %d is empty or leaves the box [%g, %g)", W.lo[d], W.hi[d], d, c->g.bmin[d], c->g.bmax[d]);
	}
	HIPCHK(c, hipStreamSynchronize(c->stream));
	widom_free(c);
	// one buffer {r[n][3], q[n][4], dU[n], sum_w[slabs], count[slabs]}
	const size_t n = instances, words = 8 * n + 2 * (size_t)slabs;
	int rc = dalloc(c, &c->d_widom, words);
	if (rc) return rc;
	HIPCHK(c, hipMemsetAsync(c->d_widom, 0, words * sizeof(double), c->stream));
	W.n = instances;
	W.slabs = slabs;
	W.rotates = c->h_ct.rotdof[component] > 0;
	W.seed = seed;
	W.len_y = c->global_len[1];
	W.temperature = temperature;
	W.r = c->d_widom;
	W.q = W.r + 3 * n;
	W.dU = W.q + 4 * n;
	W.sum_w = W.dU + n;
	W.count = (unsigned long long*)(W.sum_w + slabs);
	c->wd = W;
	c->wd_comp = component;
	return LS1HIP_OK;
}

// one sample; the caller has checked nothing
int widom_sample_impl(ls1hip_ctx* c) {
	REQUIRE(c, c->wd.n > 0 && c->d_widom, "Widom sampling is not configured (ls1hip_widom_config)");
	InsertParams P;
	int rc = insert_params(c, &P);
	if (rc) return rc;
	REQUIRE(c, c->wd_comp < c->h_ct.ncomp, "the component set changed since ls1hip_widom_config");
	WidomParams W = c->wd;
	W.sample = c->wd_samples;
	launch_widom_generate(W, c->stream);
	P.n = W.n;
	P.comp = c->wd_comp;
	P.tr = W.r;
	P.tq = W.q;
	P.dU = W.dU;
	if ((rc = insert_launch(c, P))) return rc;
	launch_widom_accumulate(W, c->stream);
	HIPCHK(c, hipGetLastError());
	c->wd_samples++;
	c->wd_last = W.n;
	return LS1HIP_OK;
}

extern "C" int ls1hip_widom_sample(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	HIPCHK(c, hipSetDevice(c->device));
	return widom_sample_impl(c);
}

extern "C" int ls1hip_widom_read(ls1hip_ctx* c, size_t cap_slabs, double* sum_w, uint64_t* n, uint64_t* samples) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->wd.n > 0 && c->d_widom, "Widom sampling is not configured (ls1hip_widom_config)");
	REQUIRE(c, (!sum_w && !n) || cap_slabs >= (size_t)c->wd.slabs, "buffer too small: %zu < %d slabs", cap_slabs, c->wd.slabs);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (sum_w) HIPCHK(c, hipMemcpy(sum_w, c->wd.sum_w, (size_t)c->wd.slabs * sizeof(double), hipMemcpyDeviceToHost));
	if (n) HIPCHK(c, hipMemcpy(n, c->wd.count, (size_t)c->wd.slabs * sizeof(uint64_t), hipMemcpyDeviceToHost));
	if (samples) *samples = c->wd_samples;
	return LS1HIP_OK;
}

extern "C" int ls1hip_widom_last(ls1hip_ctx* c, size_t cap, double* r, double* q, double* dU, size_t* n) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->wd.n > 0 && c->d_widom, "Widom sampling is not configured (ls1hip_widom_config)");
	const size_t have = c->wd_last;
	if (n) *n = have;
	if ((!r && !q && !dU) || have == 0) return LS1HIP_OK;
	REQUIRE(c, cap >= have, "buffer too small: %zu < %zu tests", cap, have);
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (r) HIPCHK(c, hipMemcpy(r, c->wd.r, have * 3 * sizeof(double), hipMemcpyDeviceToHost));
	if (q) HIPCHK(c, hipMemcpy(q, c->wd.q, have * 4 * sizeof(double), hipMemcpyDeviceToHost));
	if (dU) HIPCHK(c, hipMemcpy(dU, c->wd.dU, have * sizeof(double), hipMemcpyDeviceToHost));
	return LS1HIP_OK;
}

extern "C" int ls1hip_widom_reset(ls1hip_ctx* c) {
	if (!c) return LS1HIP_EINVAL;
	REQUIRE(c, c->wd.n > 0 && c->d_widom, "Widom sampling is not configured (ls1hip_widom_config)");
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipMemsetAsync(c->wd.sum_w, 0, 2 * (size_t)c->wd.slabs * sizeof(double), c->stream));
	c->wd_samples = 0;
	return LS1HIP_OK;
}
