// Stand-alone check of dma_run_split (ls1-mardyn_amd/csrc/dma_run.hpp): the split of the region rows' runs between the dword and the
// 16-byte LDS-DMA form, driven over random regions — cell counts 0 .. 40, runs interrupted at arbitrary cells, global starts of either
// parity.  The copy is replayed lane by lane exactly as stage_positions_dma issues it; asserted: the 16-byte body starts on an even
// LDS slot, no instruction writes outside its own run, every molecule of the region lands exactly once in its slot (slot = prefix sum
// of the cell counts) from its own global index, slots of no molecule stay untouched, and the instruction count per run.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/hostcpp/dma_run_check.cpp -o dma_run_check
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../ls1-mardyn_amd/csrc/dma_run.hpp"

#define CHECK(c)                                                            \
	do {                                                                    \
		if (!(c)) {                                                         \
			std::fprintf(stderr, "line %d: %s (seed %u)\n", __LINE__, #c, seed); \
			return 1;                                                       \
		}                                                                   \
	} while (0)

int main(int argc, char** argv) {
	const int regions = argc > 1 ? std::atoi(argv[1]) : 20000;
	constexpr int RX = 6, ROWS = 24;  // the list kernels' region: 6 x 6 x 4 cells
	uint64_t runs_total = 0, inst16 = 0, inst4 = 0, inst_dword_only = 0;
	for (unsigned seed = 1; seed <= (unsigned)regions; ++seed) {
		std::mt19937 rng(seed);
		const int maxc = (seed % 3 == 0) ? 40 : (seed % 3 == 1 ? 20 : 3);  // crowded, liquid-like, nearly empty (many zero cells)
		std::vector<uint32_t> cnt(ROWS * RX), cstart(ROWS * RX + 1), gbeg(ROWS * RX);
		uint32_t g = rng() % 1000u, tot = 0;
		for (int c = 0; c < ROWS * RX; ++c) {
			cnt[c] = rng() % (uint32_t)(maxc + 1);
			if (c % RX == 0 || rng() % 4u == 0u) g += 1u + rng() % 500u;  // a new row, or a halo cell / domain face: the run breaks
			gbeg[c] = g;
			g += cnt[c];
			cstart[c] = tot;
			tot += cnt[c];
		}
		cstart[ROWS * RX] = tot;
		std::vector<int> written(tot + 8, 0);
		std::vector<uint32_t> src(tot + 8, 0xffffffffu);
		auto write = [&](uint32_t slot, uint32_t gi, uint32_t lo, uint32_t hi) {  // one molecule into `slot`; the run owns [lo, hi)
			if (slot < lo || slot >= hi || slot >= written.size()) return false;
			++written[slot];
			src[slot] = gi;
			return true;
		};
		auto copy_run = [&](uint32_t s0, uint32_t g0, uint32_t n) {
			const ls1::DmaRunSplit sp = ls1::dma_run_split(s0, n);
			if (sp.head + 2u * sp.pairs + sp.tail != n || sp.head > 1u || sp.tail > 1u) return false;
			if (sp.pairs && ((s0 + sp.head) & 1u)) return false;  // the body's LDS side starts on an even slot
			uint32_t s = s0, gi = g0;
			if (sp.head && !write(s, gi, s0, s0 + n)) return false;
			s += sp.head;
			gi += sp.head;
			for (uint32_t k0 = 0; k0 < sp.pairs; k0 += 64u)
				for (uint32_t lane = 0; lane < 64u; ++lane) {
					const uint32_t q = k0 + lane;
					if (q >= sp.pairs) continue;  // EXEC-masked
					if (!write(s + 2u * k0 + 2u * lane, gi + 2u * q, s0, s0 + n)) return false;  // LDS: wave-uniform base + lane * 16
					if (!write(s + 2u * k0 + 2u * lane + 1u, gi + 2u * q + 1u, s0, s0 + n)) return false;
				}
			if (sp.tail && !write(s + 2u * sp.pairs, gi + 2u * sp.pairs, s0, s0 + n)) return false;
			++runs_total;
			inst16 += (sp.pairs + 63u) / 64u;
			inst4 += sp.head + sp.tail;
			inst_dword_only += (2u * n + 63u) / 64u;
			return ls1::dma_run_instructions(sp) == sp.head + (sp.pairs + 63u) / 64u + sp.tail;
		};
		// the run detection of stage_positions_dma
		for (int r = 0; r < ROWS; ++r) {
			const uint32_t* cs = &cstart[r * RX];
			const uint32_t* gb = &gbeg[r * RX];
			uint32_t run_s = cs[0], run_g = gb[0], run_n = 0;
			for (int c = 0; c < RX; ++c) {
				const uint32_t n = cs[c + 1] - cs[c];
				if (gb[c] != run_g + run_n) {
					if (run_n) CHECK(copy_run(run_s, run_g, run_n));
					run_s = cs[c];
					run_g = gb[c];
					run_n = 0;
				}
				run_n += n;
			}
			if (run_n) CHECK(copy_run(run_s, run_g, run_n));
		}
		for (int c = 0; c < ROWS * RX; ++c)
			for (uint32_t k = 0; k < cnt[c]; ++k) {
				CHECK(written[cstart[c] + k] == 1);
				CHECK(src[cstart[c] + k] == gbeg[c] + k);
			}
		for (uint32_t s = tot; s < tot + 8; ++s) CHECK(written[s] == 0);
	}
	std::printf("dma_run_check ok: %d regions, %llu runs; wave instructions per coordinate array: %llu (16-byte) + %llu (dword) against %llu dword-only\n",
				regions, (unsigned long long)runs_total, (unsigned long long)inst16, (unsigned long long)inst4, (unsigned long long)inst_dword_only);
	return 0;
}
