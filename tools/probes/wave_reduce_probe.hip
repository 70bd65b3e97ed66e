// Probe of the LDS-free wave folds (ls1-mardyn_amd/csrc/common.hpp, wave_down_f64: v_permlane32_swap / v_permlane16_swap / DPP
// row_shl) against the __shfl_down tree they replace, on the device:
//   1. wave_down_f64<O>, O = 32 .. 1: every lane < O holds the value of lane + O,
//   2. lane 0 of the sum fold and of the top-2 merge fold (store_partials of kernels_force_verlet.hip) equals lane 0 of the
//      __shfl_down form BIT FOR BIT, for random doubles incl. +-0, denormals, 1e300 and mixed magnitudes (association matters),
//   3. the sums also equal the host model (wave_reduce_model.hpp) bit for bit, the top-2 results as numbers.
// Workgroups of one wave and of eight waves.  Prints "wave_reduce_probe ok ..." and exits 0, or lists the first differences.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off tools/probes/wave_reduce_probe.hip -o wave_reduce_probe
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ls1-mardyn_amd/csrc/common.hpp"
#include "wave_reduce_model.hpp"

#define CHECK(x)                                                                         \
	do {                                                                                 \
		hipError_t e_ = (x);                                                             \
		if (e_ != hipSuccess) {                                                          \
			std::printf("%s: %s\n", #x, hipGetErrorString(e_));                          \
			return 2;                                                                    \
		}                                                                                \
	} while (0)

template <int O>
__device__ __forceinline__ void top2_step_new(double& a, double& b) {
	const double a2 = ls1::wave_down_f64<O>(a), b2 = ls1::wave_down_f64<O>(b);
	b = fmax(fmin(a, a2), fmax(b, b2));
	a = fmax(a, a2);
}

// out[wave] = {sum new, sum shfl, a new, a shfl, b new, b shfl}; down[O-index][thread] = wave_down_f64<O>(x)
__global__ void k_probe(const double* x, const double* a, const double* b, double* out, double* down, uint32_t n) {
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;  // (n is a multiple of the workgroup size: whole waves)
	const double xv = x[t], av = a[t], bv = b[t];
	down[0 * (size_t)n + t] = ls1::wave_down_f64<32>(xv);
	down[1 * (size_t)n + t] = ls1::wave_down_f64<16>(xv);
	down[2 * (size_t)n + t] = ls1::wave_down_f64<8>(xv);
	down[3 * (size_t)n + t] = ls1::wave_down_f64<4>(xv);
	down[4 * (size_t)n + t] = ls1::wave_down_f64<2>(xv);
	down[5 * (size_t)n + t] = ls1::wave_down_f64<1>(xv);
	const double s_new = ls1::wave_fold_sum(xv);
	double s_old = xv;
	for (int o = 32; o > 0; o >>= 1) s_old += __shfl_down(s_old, o);
	double a1 = av, b1 = bv;
	top2_step_new<32>(a1, b1);
	top2_step_new<16>(a1, b1);
	top2_step_new<8>(a1, b1);
	top2_step_new<4>(a1, b1);
	top2_step_new<2>(a1, b1);
	top2_step_new<1>(a1, b1);
	double a0 = av, b0 = bv;
	for (int o = 32; o > 0; o >>= 1) {
		const double a2 = __shfl_down(a0, o), b2 = __shfl_down(b0, o);
		b0 = fmax(fmin(a0, a2), fmax(b0, b2));
		a0 = fmax(a0, a2);
	}
	if ((threadIdx.x & 63) == 0) {
		double* const o = out + (size_t)(t >> 6) * 6;
		o[0] = s_new;
		o[1] = s_old;
		o[2] = a1;
		o[3] = a0;
		o[4] = b1;
		o[5] = b0;
	}
}

// which form of the offsets 32 and 16 the device code was compiled with
__global__ void k_form(int* f) {
#if defined(LS1_HAVE_PERMLANE_SWAP)
	*f = 1;
#else
	*f = 0;
#endif
}

static uint64_t bits(double d) {
	uint64_t u;
	std::memcpy(&u, &d, 8);
	return u;
}

int main() {
	using namespace wave_model;
	int bad = 0;
	size_t waves_checked = 0;
	for (int nw : {1, 8}) {
		const uint32_t blocks = 48, nt = (uint32_t)nw * 64u, n = blocks * nt, waves = n / 64u;
		Rng rng{977ull + (unsigned)nw};
		std::vector<double> x(n), a(n), b(n), out((size_t)waves * 6), down((size_t)6 * n);
		for (uint32_t i = 0; i < n; ++i) {
			x[i] = sample(rng);
			a[i] = sample(rng);
			b[i] = sample(rng);
			if ((i / 64u) & 1u) {  // odd waves: as the force pass holds them (squares, b <= a)
				a[i] = std::fabs(a[i]);
				b[i] = std::fabs(b[i]);
				if (b[i] > a[i]) std::swap(a[i], b[i]);
			}
		}
		double *dx, *da, *db, *dout, *ddown;
		CHECK(hipMalloc(&dx, n * 8));
		CHECK(hipMalloc(&da, n * 8));
		CHECK(hipMalloc(&db, n * 8));
		CHECK(hipMalloc(&dout, out.size() * 8));
		CHECK(hipMalloc(&ddown, down.size() * 8));
		CHECK(hipMemcpy(dx, x.data(), n * 8, hipMemcpyHostToDevice));
		CHECK(hipMemcpy(da, a.data(), n * 8, hipMemcpyHostToDevice));
		CHECK(hipMemcpy(db, b.data(), n * 8, hipMemcpyHostToDevice));
		hipLaunchKernelGGL(k_probe, dim3(blocks), dim3(nt), 0, 0, dx, da, db, dout, ddown, n);
		CHECK(hipGetLastError());
		CHECK(hipDeviceSynchronize());
		CHECK(hipMemcpy(out.data(), dout, out.size() * 8, hipMemcpyDeviceToHost));
		CHECK(hipMemcpy(down.data(), ddown, down.size() * 8, hipMemcpyDeviceToHost));
		for (uint32_t w = 0; w < waves; ++w) {
			const double* const o = &out[(size_t)w * 6];
			const uint32_t t0 = w * 64u;
			for (int k = 0; k < 6; ++k) {
				const uint32_t off = 32u >> k;
				for (uint32_t l = 0; l < off; ++l)
					if (bits(down[(size_t)k * n + t0 + l]) != bits(x[t0 + l + off]) && bad++ < 10)
						std::printf("waves/wg %d wave %u: wave_down_f64<%u> lane %u = %a, lane %u holds %a\n", nw, w, off, l,
									down[(size_t)k * n + t0 + l], l + off, x[t0 + l + off]);
			}
			if ((bits(o[0]) != bits(o[1]) || bits(o[2]) != bits(o[3]) || bits(o[4]) != bits(o[5])) && bad++ < 10)
				std::printf("waves/wg %d wave %u: new / shfl  sum %a / %a  a %a / %a  b %a / %a\n", nw, w, o[0], o[1], o[2], o[3], o[4], o[5]);
			const double ms = fold_sum(&x[t0], true);
			const Top2 mt = fold_top2(&a[t0], &b[t0], true);
			if ((bits(ms) != bits(o[0]) || mt.a != o[2] || mt.b != o[4]) && bad++ < 10)
				std::printf("waves/wg %d wave %u: device / model  sum %a / %a  a %a / %a  b %a / %a\n", nw, w, o[0], ms, o[2], mt.a, o[4], mt.b);
			++waves_checked;
		}
		CHECK(hipFree(dx));
		CHECK(hipFree(da));
		CHECK(hipFree(db));
		CHECK(hipFree(dout));
		CHECK(hipFree(ddown));
	}
	if (bad) {
		std::printf("wave_reduce_probe FAILED: %d differences\n", bad);
		return 1;
	}
	int *dform, hform = -1;
	CHECK(hipMalloc(&dform, sizeof(int)));
	hipLaunchKernelGGL(k_form, dim3(1), dim3(1), 0, 0, dform);
	CHECK(hipMemcpy(&hform, dform, sizeof(int), hipMemcpyDeviceToHost));
	CHECK(hipFree(dform));
	const char* const form = hform == 1 ? "permlane swaps + DPP" : "shfl_down (no swap builtins) + DPP";
	std::printf("wave_reduce_probe ok: %zu waves (workgroups of 1 and 8 waves), %s\n", waves_checked, form);
	return 0;
}
