// A stand-alone host program over the C++ Grain generator of the Poseidon parameters (sylow_amd/csrc/poseidon_params.hpp): for every width
// t = 2 .. 17 it prints the round constants and the t^2 sums xs[i] + ys[j] mod r, one hexadecimal value per line.  tests/test_poseidon_params.py
// builds it with -fsanitize=address,undefined and compares the lines with the Python model, which shares nothing with this generator.
#include "../../sylow_amd/csrc/poseidon_params.hpp"

#include <cstdio>

static void put(const char* tag, int t, size_t i, const poseidon_params::U256& v) {
  printf("%s %d %zu %016llx%016llx%016llx%016llx\n", tag, t, i, (unsigned long long)v.w[3], (unsigned long long)v.w[2], (unsigned long long)v.w[1],
         (unsigned long long)v.w[0]);
}

int main() {
  for (int t = poseidon_params::T_MIN; t <= poseidon_params::T_MAX; ++t) {
    const poseidon_params::Draws d = poseidon_params::draw(t);
    if (d.constants.size() != (size_t)poseidon_params::rounds(t) * t || d.sums.size() != (size_t)t * t) return 1;
    for (size_t i = 0; i < d.constants.size(); ++i) put("C", t, i, d.constants[i]);
    for (size_t i = 0; i < d.sums.size(); ++i) put("S", t, i, d.sums[i]);
  }
  return 0;
}
