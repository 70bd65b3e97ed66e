// Stand-alone CPU check (build with -fsanitize=address,undefined) of the host model of the wave folds
// (tools/probes/wave_reduce_model.hpp): the lane-parallel fold in its __shfl_down form, the same fold with every lane >= o receiving
// poison (the LDS-free form of csrc/common.hpp: only lanes < o get the value of lane + o), and the serial evaluation of lane 0's
// expression tree must give the same bits — sum and top-2 merge; and the top-2 result must be the two largest values of its input.
//   wave_reduce_model_check [trials]
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../tools/probes/wave_reduce_model.hpp"

using namespace wave_model;

static uint64_t bits(double d) {
	uint64_t u;
	std::memcpy(&u, &d, 8);
	return u;
}

int main(int argc, char** argv) {
	const int trials = argc > 1 ? std::atoi(argv[1]) : 2000;
	Rng rng{12345};
	int bad = 0;
	for (int t = 0; t < trials && bad < 10; ++t) {
		double x[W], a[W], b[W];
		for (int i = 0; i < W; ++i) {
			x[i] = sample(rng);
			a[i] = sample(rng);
			b[i] = sample(rng);
			if (t & 1) {  // as the force pass holds them: squares, b <= a
				a[i] = std::fabs(a[i]);
				b[i] = std::fabs(b[i]);
				if (b[i] > a[i]) std::swap(a[i], b[i]);
			}
		}
		const double s0 = fold_sum(x, false), s1 = fold_sum(x, true), s2 = tree_sum(x);
		if (bits(s0) != bits(s1) || bits(s0) != bits(s2)) {
			std::printf("trial %d: sum %a %a %a\n", t, s0, s1, s2);
			++bad;
		}
		const Top2 p0 = fold_top2(a, b, false), p1 = fold_top2(a, b, true), p2 = tree_top2(a, b);
		if (bits(p0.a) != bits(p1.a) || bits(p0.b) != bits(p1.b) || bits(p0.a) != bits(p2.a) || bits(p0.b) != bits(p2.b)) {
			std::printf("trial %d: top2 {%a %a} {%a %a} {%a %a}\n", t, p0.a, p0.b, p1.a, p1.b, p2.a, p2.b);
			++bad;
		}
		if (t & 1) {
			std::vector<double> all(a, a + W);
			all.insert(all.end(), b, b + W);
			std::sort(all.begin(), all.end());
			if (p1.a != all[2 * W - 1] || p1.b != all[2 * W - 2]) {
				std::printf("trial %d: top2 {%a %a}, the two largest are {%a %a}\n", t, p1.a, p1.b, all[2 * W - 1], all[2 * W - 2]);
				++bad;
			}
		}
	}
	if (bad) return 1;
	std::printf("wave_reduce_model_check ok: %d trials\n", trials);
	return 0;
}
