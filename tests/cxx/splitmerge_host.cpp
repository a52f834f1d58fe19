// common_amd/csrc/splitmerge_math.hpp built with the host compiler (tests/test_splitmerge_cpu.py): the key and the
// streams, the anchors, the two-way log-probabilities and the log acceptance ratio of the split-merge move, as the device
// computes them.
#include <cstdint>

#include "splitmerge_math.hpp"

using namespace msc::sm;

extern "C" {

uint64_t sm_key() { return kSmKey; }
uint64_t sm_stream_stride() { return kStreamStride; }
uint64_t sm_stream_key(uint64_t seed, uint32_t stream) { return stream_key(seed, stream); }
void sm_stream_tags(uint32_t *out) {
  out[0] = kStreamProposal;
  out[1] = kStreamCoin;
  out[2] = kStreamPass0;
  out[3] = (uint32_t)kDartAccept;
}
float sm_uniform01(uint64_t key, uint64_t sweep, uint64_t row) { return uniform01(key, sweep, row); }
void sm_anchors(uint64_t seed, uint64_t sweep, uint64_t n, uint64_t *i, uint64_t *j) {
  anchors(stream_key(seed, kStreamProposal), sweep, n, i, j);
}
void sm_two_way(float s0, float s1, float *out) { two_way(s0, s1, out, out + 1, out + 2); }
double sm_log_crp_split(double log_alpha, double n0, double n1) { return log_crp_split(log_alpha, n0, n1); }
double sm_log_accept(uint32_t kind, double log_alpha, double n0, double n1, double sd0, double sd1, double sdS, double logq) {
  return log_accept(kind, log_alpha, n0, n1, sd0, sd1, sdS, logq);
}

}  // extern "C"
