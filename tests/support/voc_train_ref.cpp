// TEST INFRASTRUCTURE: the driver of tools/make_voc_train_golden.py.  Compiled there, together with the reference's DBoW2 sources and over
// oracle/ref_shims (include path only), into a temporary directory; never shipped.  One configuration per process, as the seed contract
// needs: DUtils::Random::SeedRandOnce(seed), then TemplatedVocabulary::create(features, k, L, weighting, scoring), then the node arrays
// dumped exactly (the text format loses the weights).
//   voc_train_ref IN OUT
//   IN : int32 k, L, weighting, scoring; uint32 seed; int32 ndocs; int64 offsets[ndocs + 1]; uint8 desc[offsets[ndocs]][32]
//   OUT: int64 nnodes (root included); int32 parent[nnodes]; uint8 is_leaf[nnodes]; uint8 desc[nnodes][32]; float64 weight[nnodes]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "DBoW2/FORB.h"
#include "DBoW2/TemplatedVocabulary.h"
#include "DUtils/Random.h"

typedef DBoW2::TemplatedVocabulary<DBoW2::FORB::TDescriptor, DBoW2::FORB> RefVocabulary;

struct Dump : RefVocabulary {
  void write(FILE* f) const {
    const int64_t n = (int64_t)m_nodes.size();
    fwrite(&n, 8, 1, f);
    for (const auto& nd : m_nodes) { const int32_t p = (int32_t)nd.parent; fwrite(&p, 4, 1, f); }
    for (const auto& nd : m_nodes) { const uint8_t l = nd.isLeaf() ? 1 : 0; fwrite(&l, 1, 1, f); }
    for (const auto& nd : m_nodes) {
      uint8_t d[32] = {0};
      if (!nd.descriptor.empty()) std::memcpy(d, nd.descriptor.template ptr<unsigned char>(), 32);
      fwrite(d, 1, 32, f);
    }
    for (const auto& nd : m_nodes) { const double w = nd.weight; fwrite(&w, 8, 1, f); }
  }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[4], ndocs = 0;
  uint32_t seed = 0;
  if (fread(hdr, 4, 4, in) != 4 || fread(&seed, 4, 1, in) != 1 || fread(&ndocs, 4, 1, in) != 1) return 2;
  std::vector<int64_t> off(ndocs + 1);
  if (fread(off.data(), 8, off.size(), in) != off.size()) return 2;
  std::vector<std::vector<cv::Mat> > feats(ndocs);
  for (int d = 0; d < ndocs; d++)
    for (int64_t i = off[d]; i < off[d + 1]; i++) {
      cv::Mat m(1, 32, CV_8U);
      if (fread(m.ptr<unsigned char>(), 1, 32, in) != 32) return 2;
      feats[d].push_back(m);
    }
  std::fclose(in);
  DUtils::Random::SeedRandOnce((int)seed);
  Dump v;
  v.create(feats, hdr[0], hdr[1], (DBoW2::WeightingType)hdr[2], (DBoW2::ScoringType)hdr[3]);
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  v.write(out);
  std::fclose(out);
  return 0;
}
