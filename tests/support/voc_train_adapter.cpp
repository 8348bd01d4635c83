// The C++ adapter's create (include/ORBVocabulary.h) as a reference user calls it: vector<vector<cv::Mat>> in, a trained vocabulary out.
//   voc_train_adapter IN OUT   IN: the input layout of tests/support/voc_train_ref.cpp; OUT: the vocabulary's exact binary cache
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ORBVocabulary.h"

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
  ORB_SLAM3::ORBVocabulary voc;
  voc.create(feats, hdr[0], hdr[1], (DBoW2::WeightingType)hdr[2], (DBoW2::ScoringType)hdr[3], seed);
  voc.saveToBinaryFile(argv[2]);
  std::printf("words %u\n", voc.size());
  return 0;
}
