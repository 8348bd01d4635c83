// BENCH INFRASTRUCTURE: the per-pair loop through the drop-in adapter's two-camera rig SearchByBoW (include/ORBmatcher.h +
// csrc/ref_adapter/ORBmatcher.cc over liborbx.so) on the inputs of tools/rigbow_times.py.  For every pair it builds the two rig frames from
// the tool's arrays through tests/support/world_scene.h, gives both the tool's stacked FeatureVectors, makes the first a KeyFrame whose
// valid features carry a map point with mnId = the feature's stacked index, and calls SearchByBoW(KeyFrame*, Frame&, matches).  Only the
// matcher calls are timed (steady_clock).  It writes vpMapPointMatches as ids -- with these mnIds the batched call's b2a row -- and the
// return values, so that the tool can hold the two paths equal slot by slot.
//
//   rigbow_adapter_loop <in.bin> <out.bin> <passes>
// Records as tests/support/rig_bow_dump.cpp: {int32 name length, name, int32 kind (0 int32, 1 float32, 2 bytes), int32 count, data}.
#include <map>

#include "world_scene.h"

namespace {

struct Rec { int kind; std::vector<unsigned char> data; };
std::map<std::string, Rec> read_records(const char* path) {
  std::map<std::string, Rec> m;
  FILE* f = std::fopen(path, "rb");
  if (!f) return m;
  int32_t n;
  while (std::fread(&n, 4, 1, f) == 1) {
    std::string name(n, ' ');
    int32_t kind, count;
    if (std::fread(&name[0], 1, n, f) != (size_t)n || std::fread(&kind, 4, 1, f) != 1 || std::fread(&count, 4, 1, f) != 1) break;
    Rec r{kind, std::vector<unsigned char>((size_t)count * (kind == 2 ? 1 : 4))};
    if (!r.data.empty() && std::fread(r.data.data(), 1, r.data.size(), f) != r.data.size()) break;
    m[name] = std::move(r);
  }
  std::fclose(f);
  return m;
}
template <class T> const T* as(const std::map<std::string, Rec>& m, const char* name) {
  auto it = m.find(name);
  if (it == m.end()) { std::fprintf(stderr, "missing record %s\n", name); std::exit(2); }
  return (const T*)it->second.data.data();
}
void write_rec(FILE* f, const std::string& name, int kind, const void* p, size_t count) {
  const int32_t n = (int32_t)name.size(), k = kind, c = (int32_t)count;
  std::fwrite(&n, 4, 1, f); std::fwrite(name.data(), 1, name.size(), f); std::fwrite(&k, 4, 1, f); std::fwrite(&c, 4, 1, f);
  if (count) std::fwrite(p, kind == 2 ? 1 : 4, count, f);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: rigbow_adapter_loop <in.bin> <out.bin> <passes>\n"); return 2; }
  const auto in = read_records(argv[1]);
  const int passes = std::atoi(argv[3]);
  const int32_t* shape = as<int32_t>(in, "shape");   // frames, features a side, pairs, image size
  const int NF = shape[0], n = shape[1], P = shape[2], size = shape[3], cap = 2 * n;
  const float ratio = as<float>(in, "call")[0];
  const cv::KeyPoint* kl = as<cv::KeyPoint>(in, "kps_l");
  const cv::KeyPoint* kr = as<cv::KeyPoint>(in, "kps_r");
  const unsigned char *dl = as<unsigned char>(in, "desc_l"), *dr = as<unsigned char>(in, "desc_r"), *valid = as<unsigned char>(in, "valid");
  const int32_t *pairs = as<int32_t>(in, "pairs"), *fv_node = as<int32_t>(in, "fv_node"), *fv_ptr = as<int32_t>(in, "fv_ptr"),
                *fv_feat = as<int32_t>(in, "fv_feat"), *fv_n = as<int32_t>(in, "fv_n");

  World w;
  w.rows = size; w.cols = size; w.nlevels = 8;
  w.scale.resize(8); w.sigma2.resize(8); w.inv_sigma2.resize(8);
  for (int l = 0; l < 8; l++) { w.scale[l] = l ? w.scale[l - 1] * 1.2f : 1.f; w.sigma2[l] = w.scale[l] * w.scale[l]; w.inv_sigma2[l] = 1.f / w.sigma2[l]; }
  w.logScaleFactor = std::log(1.2f);
  w.views.resize(4);
  auto fill = [&](int v0, int f) {
    for (int c = 0; c < 2; c++) {
      View& V = w.views[v0 + c];
      V.n = n;
      V.kps.assign((c ? kr : kl) + (size_t)f * n, (c ? kr : kl) + (size_t)(f + 1) * n);
      V.desc = cv::Mat(n, 32, CV_8U);
      std::memcpy(V.desc.data, (c ? dr : dl) + (size_t)f * n * 32, (size_t)n * 32);
      V.fv.clear();
    }
  };
  auto feat_vec = [&](int f) {
    DBoW2::FeatureVector fv;
    const int32_t* ptr = fv_ptr + (size_t)f * (cap + 1);
    for (int j = 0; j < fv_n[f]; j++) {
      std::vector<unsigned int>& v = fv[(unsigned)fv_node[(size_t)f * cap + j]];
      for (int k = ptr[j]; k < ptr[j + 1]; k++) v.push_back((unsigned)fv_feat[(size_t)f * cap + k]);
    }
    return fv;
  };

  std::vector<int32_t> ids((size_t)P * cap, -1), ret(P, 0);
  std::vector<float> ms;
  for (int pass = 0; pass < passes; pass++) {
    double t = 0;
    for (int p = 0; p < P; p++) {
      const int fa = pairs[2 * p], fb = pairs[2 * p + 1];
      (void)NF;
      fill(0, fa); fill(2, fb);
      Scene s(w, false);
      Frame Fk, F;
      s.make_rig_frame(Fk, 0, 1, s.pose(0));
      s.make_rig_frame(F, 2, 3, s.pose(0));
      Fk.mFeatVec = feat_vec(fa);
      F.mFeatVec = feat_vec(fb);
      KeyFrame* K = s.make_keyframe(Fk);
      std::vector<MapPoint> pts(K->N);
      for (int i = 0; i < K->N; i++) {
        pts[i].mnId = i;
        if (valid[(size_t)fa * cap + i]) K->mvpMapPoints[i] = &pts[i];
      }
      std::vector<MapPoint*> matches;
      ORBmatcher matcher(ratio, true);
      const auto t0 = std::chrono::steady_clock::now();
      const int r = matcher.SearchByBoW(K, F, matches);
      t += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (pass == 0) {
        ret[p] = r;
        for (size_t i = 0; i < matches.size() && i < (size_t)cap; i++) ids[(size_t)p * cap + i] = (int32_t)mp_id(matches[i]);
      }
    }
    ms.push_back((float)t);
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  write_rec(o, "ids", 0, ids.data(), ids.size());
  write_rec(o, "ret", 0, ret.data(), ret.size());
  write_rec(o, "ms", 1, ms.data(), ms.size());
  std::fclose(o);
  return 0;
}
