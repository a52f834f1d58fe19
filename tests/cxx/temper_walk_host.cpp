// Host build of the walk k_chains_exchange makes (common_amd/csrc/temper_math.hpp exchange_ladder, one call per ladder) and
// of the annealing step, driven from tests/test_temper_cpu.py: the arrays come in on stdin and go out on stdout as raw
// words, so that the test can hold the C++ the kernels run to its numpy restatement on the same uniforms.
//   in:  uint64 {nladders, nrungs, nfeat, ld_joint, parity}; double joint[nchains][ld_joint]; float beta[nchains];
//        int32 rung[nchains]; float u[nchains] (the uniform of pair j of ladder l at l * nrungs + j);
//        uint32 proposed[npairs], accepted[npairs]; float beta_to[nchains]; double logw[nchains]
//   out: float beta[nchains]; int32 rung[nchains]; uint32 proposed[npairs], accepted[npairs]; uint32 ok[nladders];
//        double logw[nchains] after anneal_step(beta as it came in -> beta_to)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "temper_math.hpp"

using namespace msc::temper;

struct TableUniform {
  const float *u;
  float operator()(uint32_t j) const { return u[j]; }
};

template <class T>
static bool get(std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, stdin) == n;
}
template <class T>
static void put(const std::vector<T> &v) {
  if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), stdout);
}

int main() {
  std::vector<uint64_t> h;
  if (!get(h, 5)) return 2;
  const uint64_t nl = h[0], R = h[1], ld = h[3], parity = h[4], nc = nl * R, np = nl * ladder_pairs((uint32_t)R);
  const uint32_t F = (uint32_t)h[2];
  std::vector<double> joint, logw;
  std::vector<float> beta, u, beta_to;
  std::vector<int32_t> rung;
  std::vector<uint32_t> prop, acc, ok(nl);
  if (!get(joint, nc * ld) || !get(beta, nc) || !get(rung, nc) || !get(u, nc) || !get(prop, np) || !get(acc, np) ||
      !get(beta_to, nc) || !get(logw, nc))
    return 2;
  for (uint64_t c = 0; c < nc; c++) anneal_step(beta[c], beta_to[c], chain_loglik(joint.data() + c * ld, F), &logw[c]);
  for (uint64_t l = 0; l < nl; l++)
    ok[l] = exchange_ladder(joint.data() + l * R * ld, ld, F, (uint32_t)R, beta.data() + l * R, rung.data() + l * R, parity,
                            TableUniform{u.data() + l * R}, prop.data() + l * (R - 1), acc.data() + l * (R - 1));
  put(beta);
  put(rung);
  put(prop);
  put(acc);
  put(ok);
  put(logw);
  return 0;
}
