// Semantics probe of the gfx950 LDS-DMA loads used for the region staging of the list force pass (global_load_lds_dword and
// global_load_lds_dwordx4): per-lane global source, wave-uniform LDS base + lane * size, EXEC-masked lanes write nothing, runs of
// doubles land bit-exactly — dword-wise at any 8-byte alignment; with the 16-byte form split as stage_positions_dma splits a run
// (dma_run.hpp): an odd first LDS slot dword-wise, the body from an even LDS slot with the 16-byte form (EXEC-masked last
// instruction) whatever the parity of the GLOBAL index (16-byte and only 8-byte aligned dwordx4 sources), an odd last molecule
// dword-wise.  CROSS-WAVE: wave w copies the row that wave w + 1 reads, behind s_waitcnt vmcnt(0) + barrier (the data of a DMA is an
// LDS write pending on vmcnt).
//   hipcc --offload-arch=gfx950 -O2 tools/probes/glds_probe.hip -o tools/probes/glds_probe
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>

typedef __attribute__((address_space(3))) void* lds_ptr;
typedef const __attribute__((address_space(1))) void* glb_ptr;

constexpr int NW = 4, ROW = 256;

__device__ __forceinline__ void copy_dwords(const double* g, double* l, uint32_t nd, int lane) {
	for (uint32_t k0 = 0; k0 < nd; k0 += 64u) {
		const uint32_t d = k0 + (uint32_t)lane;
		if (d < nd)
			__builtin_amdgcn_global_load_lds((glb_ptr)(reinterpret_cast<const uint32_t*>(g) + d), (lds_ptr)(reinterpret_cast<uint32_t*>(l) + k0), 4, 0, 0);
	}
}

// mode 0: dword form; 1: the staging's split (head / tail by the LDS slot alone, 16-byte body)
struct Case {
	int n[NW], src_off[NW], dst_off[NW];
};
__global__ void __launch_bounds__(NW * 64) k(const double* src, double* out, Case c, int mode) {
	__shared__ __attribute__((aligned(16))) double s[NW * ROW];
	const int tid = threadIdx.x, lane = tid & 63;
	const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
	for (int i = tid; i < NW * ROW; i += NW * 64) s[i] = -1.0;
	__syncthreads();
	{
		uint32_t n = (uint32_t)c.n[wv];
		const uint32_t s0 = (uint32_t)c.dst_off[wv], g0 = (uint32_t)c.src_off[wv];
		const double* g = src + g0;
		double* l = s + wv * ROW + s0;
		if (mode == 0) {
			copy_dwords(g, l, 2u * n, lane);
		} else if (n) {
			if (s0 & 1u) {
				copy_dwords(g, l, 2u, lane);
				++g; ++l; --n;
			}
			const uint32_t np = n >> 1;
			for (uint32_t k0 = 0; k0 < np; k0 += 64u) {
				const uint32_t q = k0 + (uint32_t)lane;
				if (q < np) __builtin_amdgcn_global_load_lds((glb_ptr)(g + 2u * q), (lds_ptr)(l + 2u * k0), 16, 0, 0);
			}
			if (n & 1u) copy_dwords(g + (n - 1u), l + (n - 1u), 2u, lane);
		}
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
	__syncthreads();
	// wave w + 1 reads (and hands out) the row wave w copied
	const int row = (wv + NW - 1) % NW;
	for (int i = lane; i < ROW; i += 64) out[row * ROW + i] = s[row * ROW + i];
}

int main() {
	const int N = 4096;
	std::vector<double> h(N), o(NW * ROW);
	for (int i = 0; i < N; ++i) h[i] = 1000.0 + i + 1.0 / (i + 3);
	double *d, *dout;
	if (hipMalloc(&d, N * sizeof(double)) != hipSuccess || hipMalloc(&dout, NW * ROW * sizeof(double)) != hipSuccess) return 2;
	if (hipMemcpy(d, h.data(), N * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return 2;
	// per wave {n}, {src_off}, {dst_off}; n + dst_off <= ROW.  Equal parities: even / even and odd / odd starts, even and odd
	// lengths (head, tail, both, neither), bodies of less than one, exactly one (128 molecules) and more than one instruction
	const Case cases[] = {
		{{100, 97, 33, 64}, {6, 1, 12, 0}, {2, 5, 0, 0}},
		{{1, 2, 3, 200}, {3, 3, 8, 5}, {9, 9, 2, 11}},
		{{128, 129, 130, 131}, {0, 0, 1, 1}, {0, 0, 1, 1}},
		{{127, 126, 255, 256}, {7, 7, 1, 0}, {1, 1, 1, 0}},
		{{0, 94, 17, 31}, {4, 21, 40, 2}, {4, 3, 2, 0}},
	};
	// unequal parities of LDS slot and global index: the 16-byte body reads from an 8-byte aligned source
	const Case mixed[] = {
		{{100, 97, 33, 64}, {7, 2, 13, 1}, {2, 5, 0, 0}},
		{{1, 2, 3, 200}, {4, 2, 9, 4}, {9, 9, 2, 11}},
	};
	auto run = [&](const Case& c, int mode, const char* what) {
		int bad = 0;
		hipLaunchKernelGGL(k, dim3(1), dim3(NW * 64), 0, 0, d, dout, c, mode);
		if (hipMemcpy(o.data(), dout, NW * ROW * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 1000000;
		for (int w = 0; w < NW; ++w)
			for (int i = 0; i < ROW; ++i) {
				const double want = (i >= c.dst_off[w] && i < c.dst_off[w] + c.n[w]) ? h[c.src_off[w] + i - c.dst_off[w]] : -1.0;
				if (o[w * ROW + i] != want) {
					if (bad < 5) printf("%s wave %d n=%d src_off=%d dst_off=%d: s[%d] = %.17g, want %.17g\n", what, w, c.n[w], c.src_off[w], c.dst_off[w], i, o[w * ROW + i], want);
					++bad;
				}
			}
		return bad;
	};
	int bad = 0, ncase = 0;
	for (auto& c : cases) {
		bad += run(c, 0, "dword form");
		bad += run(c, 1, "16-byte form");
		ncase += 2;
	}
	for (auto& c : mixed) {
		bad += run(c, 0, "dword form");
		bad += run(c, 1, "16-byte form, 8-byte aligned source");
		ncase += 2;
	}
	printf(bad ? "glds probe: %d mismatches\n" : "glds probe ok (%d launches, 4 waves each, cross-wave)\n", bad ? bad : ncase);
	return bad != 0;
}
