// TEST INFRASTRUCTURE: the two-camera rig SearchByBoW scenarios of tests/support/matcher_world.cpp -- bow_kf_frame_rig (:124-146, variant
// 1) and bow_kf_kf_rig (:148-172, variant 1): the same frames, keyframes, points and bindings, built from the same world through
// world_scene.h -- written flattened as the stacked sides of include/orbx_rigbow.h (left keypoints, right keypoints, the stacked
// descriptors, the FeatureVector as node / ptr / feat arrays, the valid flag and the mnId of every feature's map point), so that
// tests/rigbow_model.py and liborbx_rigbow.so can be held to the vpMapPointMatches / vpMatches12 lines the reference printed for them
// (tests/golden/matcher_world_ref.txt.gz).  The drop-in adapter (include/ORBmatcher.h + csrc/ref_adapter/ORBmatcher.cc, here on the
// oracle-backed stub of the C-ABI) is run on the same objects; its result is written beside the sides.  Needs nothing from the reference.
//
//   rig_bow_dump <world.bin> <out.bin>
// out.bin: records {int32 name length, name, int32 kind (0 int32, 1 float32, 2 bytes), int32 count, data}.
#include "world_scene.h"

namespace {

struct Dump {
  FILE* f;
  void rec(const std::string& name, int kind, const void* p, size_t count, size_t elem) {
    const int32_t n = (int32_t)name.size(), k = kind, c = (int32_t)count;
    std::fwrite(&n, 4, 1, f); std::fwrite(name.data(), 1, name.size(), f); std::fwrite(&k, 4, 1, f); std::fwrite(&c, 4, 1, f);
    if (count) std::fwrite(p, elem, count, f);
  }
  void ints(const std::string& name, const std::vector<int32_t>& v) { rec(name, 0, v.data(), v.size(), 4); }
  void floats(const std::string& name, const std::vector<float>& v) { rec(name, 1, v.data(), v.size(), 4); }
  void bytes(const std::string& name, const void* p, size_t n) { rec(name, 2, p, n, 1); }
};

// one stacked side: `points` are the features' map points (NULL: none); a feature is valid when it has a point that is not bad
void dump_side(Dump& d, const std::string& tag, int nleft, int nright, const std::vector<cv::KeyPoint>& kl, const std::vector<cv::KeyPoint>& kr,
               const cv::Mat& desc, const DBoW2::FeatureVector& fv, const std::vector<MapPoint*>& points) {
  d.ints(tag + "counts", {nleft, nright});
  d.bytes(tag + "kps_l", kl.data(), kl.size() * sizeof(cv::KeyPoint));
  d.bytes(tag + "kps_r", kr.data(), kr.size() * sizeof(cv::KeyPoint));
  d.bytes(tag + "desc", desc.data, (size_t)(nleft + nright) * 32);   // left rows, then right rows
  std::vector<int32_t> node, ptr(1, 0), feat;
  for (const auto& kv : fv) {
    node.push_back((int32_t)kv.first);
    for (unsigned f : kv.second) feat.push_back((int32_t)f);
    ptr.push_back((int32_t)feat.size());
  }
  d.ints(tag + "fv_node", node);
  d.ints(tag + "fv_ptr", ptr);
  d.ints(tag + "fv_feat", feat);
  std::vector<int32_t> ids, valid;
  for (MapPoint* p : points) { ids.push_back((int32_t)mp_id(p)); valid.push_back(p && !p->isBad()); }
  d.ints(tag + "mnid", ids);
  d.ints(tag + "valid", valid);
}

void result(Dump& d, const std::string& tag, int ret, const std::vector<MapPoint*>& v) {
  d.ints(tag + "ret", {ret});
  std::vector<int32_t> ids;
  for (MapPoint* p : v) ids.push_back((int32_t)mp_id(p));
  d.ints(tag + "ids", ids);
}

// bow_kf_frame_rig: matcher_world.cpp:124-146, variant 1
void frame_scenario(Dump& d, const World& w) {
  Scene s(w, false);
  Frame Fk, F;
  s.make_rig_frame(Fk, 0, 1, s.pose(0));
  s.make_rig_frame(F, 2, 3, s.pose(4));
  KeyFrame* K = s.make_keyframe(Fk);
  s.make_points(s.mps, 0, s.pose(0), 0, 0);
  s.make_points(s.mpsB, 1, Fk.GetRelativePoseTrl() * Fk.GetPose(), 100000, 3);
  for (int i = 0; i < K->N; i++) {
    MapPoint* p = i < (int)s.mps.size() ? &s.mps[i] : &s.mpsB[i - (int)s.mps.size()];
    if (H(i, 50) % 4 != 0) K->mvpMapPoints[i] = p;
  }
  const std::string tag = "frame.";
  dump_side(d, tag + "a.", K->NLeft, K->NRight, K->mvKeys, K->mvKeysRight, K->mDescriptors, K->mFeatVec, K->mvpMapPoints);
  dump_side(d, tag + "b.", F.Nleft, F.Nright, F.mvKeys, F.mvKeysRight, F.mDescriptors, F.mFeatVec, F.mvpMapPoints);
  d.floats(tag + "call", {0.7f, 1.0f});   // mfNNratio, mbCheckOrientation
  std::vector<MapPoint*> matches;
  ORBmatcher matcher(0.7, true);
  const int ret = matcher.SearchByBoW(K, F, matches);
  result(d, tag + "adapter.", ret, matches);
}

// bow_kf_kf_rig: matcher_world.cpp:148-172, variant 1
void keyframes_scenario(Dump& d, const World& w) {
  Scene s(w, false);
  Frame F1, F2;
  s.make_rig_frame(F1, 0, 1, s.pose(0));
  s.make_rig_frame(F2, 2, 3, s.pose(4));
  KeyFrame *K1 = s.make_keyframe(F1), *K2 = s.make_keyframe(F2);
  s.make_points(s.mps, 0, s.pose(0), 0, 0);
  s.make_points(s.mpsB, 2, s.pose(4), 100000, 5);
  for (int i = 0; i < (int)s.mps.size(); i++) if (H(i, 60) % 4 != 0) K1->mvpMapPoints[i] = &s.mps[i];
  for (int i = 0; i < (int)s.mpsB.size(); i++) if (H(i, 61) % 5 != 0) K2->mvpMapPoints[i] = &s.mpsB[i];
  for (int i = (int)s.mps.size(); i < K1->N; i += 3) K1->mvpMapPoints[i] = &s.mps[i % s.mps.size()];
  for (int i = (int)s.mpsB.size(); i < K2->N; i += 2) K2->mvpMapPoints[i] = &s.mpsB[i % s.mpsB.size()];
  const std::string tag = "keyframes.";
  dump_side(d, tag + "a.", K1->NLeft, K1->NRight, K1->mvKeys, K1->mvKeysRight, K1->mDescriptors, K1->mFeatVec, K1->mvpMapPoints);
  dump_side(d, tag + "b.", K2->NLeft, K2->NRight, K2->mvKeys, K2->mvKeysRight, K2->mDescriptors, K2->mFeatVec, K2->mvpMapPoints);
  d.floats(tag + "call", {0.9f, 1.0f});
  std::vector<MapPoint*> m12;
  ORBmatcher matcher(0.9, true);
  const int ret = matcher.SearchByBoW(K1, K2, m12);
  result(d, tag + "adapter.", ret, m12);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: rig_bow_dump <world.bin> <out.bin>\n"); return 2; }
  World w;
  if (!load_world(argv[1], w) || w.views.size() < 4) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  Dump d{std::fopen(argv[2], "wb")};
  if (!d.f) return 2;
  frame_scenario(d, w);
  keyframes_scenario(d, w);
  std::fclose(d.f);
  return 0;
}
