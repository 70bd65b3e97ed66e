// Host model (plain C++, no GPU) of the wave folds of the reduction kernels (ls1-mardyn_amd/csrc/common.hpp, wave_down_f64):
//   for (o = 32; o > 0; o >>= 1) v = op(v, value of lane + o)
// in two forms — the __shfl_down one (a lane without a source gets its own value back) and the LDS-free one, where only lanes < o
// receive the value of lane + o and every other lane receives something unspecified (modelled as a quiet NaN: if it ever reached
// lane 0 the result would show it).  Lane 0 is the result.  tree_* evaluate lane 0's expression tree directly, by recursion, as the
// serial reference of the same association order.
// Used by tools/probes/wave_reduce_probe.hip (against the device) and tests/hostcpp/wave_reduce_model_check.cpp (on the CPU).
#pragma once
#include <cmath>
#include <limits>

namespace wave_model {

constexpr int W = 64;

struct Top2 {
	double a, b;  // the largest and the second largest value
};
inline Top2 merge_top2(Top2 x, Top2 y) {  // store_partials: b = fmax(fmin(a, a2), fmax(b, b2)); a = fmax(a, a2)
	Top2 r;
	r.b = std::fmax(std::fmin(x.a, y.a), std::fmax(x.b, y.b));
	r.a = std::fmax(x.a, y.a);
	return r;
}

// source value of lane i at offset o: poison = false, the __shfl_down form; true, the LDS-free form
template <class T>
inline T down(const T* v, int i, int o, bool poison, T bad) {
	if (poison) return i < o ? v[i + o] : bad;
	return i + o < W ? v[i + o] : v[i];
}

inline double fold_sum(const double* x, bool poison) {
	double v[W], t[W];
	for (int i = 0; i < W; ++i) v[i] = x[i];
	for (int o = W / 2; o > 0; o >>= 1) {
		for (int i = 0; i < W; ++i) t[i] = down(v, i, o, poison, std::numeric_limits<double>::quiet_NaN());
		for (int i = 0; i < W; ++i) v[i] = v[i] + t[i];
	}
	return v[0];
}
inline Top2 fold_top2(const double* a, const double* b, bool poison) {
	Top2 v[W], t[W];
	const double nan = std::numeric_limits<double>::quiet_NaN();
	for (int i = 0; i < W; ++i) v[i] = {a[i], b[i]};
	for (int o = W / 2; o > 0; o >>= 1) {
		for (int i = 0; i < W; ++i) t[i] = down(v, i, o, poison, Top2{nan, nan});
		for (int i = 0; i < W; ++i) v[i] = merge_top2(v[i], t[i]);
	}
	return v[0];
}

// lane i's value before the step of offset o (o = W: the input), by recursion over the tree
inline double tree_sum(const double* x, int i = 0, int o = 1) {
	if (o == W) return x[i];
	return tree_sum(x, i, 2 * o) + tree_sum(x, i + o, 2 * o);
}
inline Top2 tree_top2(const double* a, const double* b, int i = 0, int o = 1) {
	if (o == W) return {a[i], b[i]};
	return merge_top2(tree_top2(a, b, i, 2 * o), tree_top2(a, b, i + o, 2 * o));
}

// test values: +-0, denormals, 1e300, and magnitudes mixed so that the association order shows in the sum's bits
struct Rng {
	unsigned long long s;
	unsigned next() {
		s = s * 6364136223846793005ull + 1442695040888963407ull;
		return (unsigned)(s >> 33);
	}
	double uni() { return (next() + 0.5) / 2147483648.0; }
};
inline double sample(Rng& r) {
	const unsigned k = r.next() % 16u;
	const double sgn = (r.next() & 1u) ? -1. : 1.;
	switch (k) {
		case 0: return sgn * 0.;
		case 1: return sgn * 4.9406564584124654e-324 * (double)(1u + r.next() % 1000u);  // denormals
		case 2: return sgn * 2.2250738585072014e-308 * r.uni();                             // denormals up to DBL_MIN
		case 3: return sgn * 1e300 * r.uni();
		case 4: return sgn * 1e-300 * r.uni();
		case 5: return sgn * std::ldexp(r.uni(), (int)(r.next() % 200u) - 100);
		case 6: return sgn * 1e16 * r.uni();
		case 7: return sgn * 1.;
		default: return sgn * r.uni() * (k < 12 ? 1. : 1e3);
	}
}

}  // namespace wave_model
