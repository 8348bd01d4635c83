// TEST INFRASTRUCTURE: the two-camera rig scenarios of tests/support/matcher_world.cpp -- proj_mp_rig (:66-85) and proj_last_rig + _wide
// (:89-121): the same frames, points, pre-bindings and track fields, built from the same world through world_scene.h -- written
// flattened in the layout of include/orbx_rigmatch.h, with the id of every point row and of every pre-bound slot, so that
// tests/rigmatch_model.py and liborbx_rigmatch.so can be held to the mvpMapPoints lines the reference printed for them
// (tests/golden/matcher_world_ref.txt.gz).  For the directions the golden does not have on a rig, the proj_last_rig frames are built
// again with a forward (tz = -0.3f) and a backward (tz = 0.3f) pose and the drop-in adapter (include/ORBmatcher.h +
// csrc/ref_adapter/ORBmatcher.cc, here on the oracle-backed stub of the C-ABI) is run on them; its result is written beside the rows.
// Needs nothing from the reference.
//
//   rig_batch_dump <world.bin> <out.bin>
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

// the rig side of a frame and the slots' holders before the call: id and Observations() of the point a slot holds, -1 without one
void dump_frame(Dump& d, const std::string& tag, const World& w, Frame& F) {
  d.ints(tag + "counts", {F.Nleft, F.Nright});
  d.bytes(tag + "kps_l", F.mvKeys.data(), F.mvKeys.size() * sizeof(cv::KeyPoint));
  d.bytes(tag + "kps_r", F.mvKeysRight.data(), F.mvKeysRight.size() * sizeof(cv::KeyPoint));
  d.bytes(tag + "desc", F.mDescriptors.data, (size_t)F.N * 32);   // left rows, then right rows
  d.ints(tag + "l2r", std::vector<int32_t>(F.mvLeftToRightMatch.begin(), F.mvLeftToRightMatch.end()));
  d.ints(tag + "r2l", std::vector<int32_t>(F.mvRightToLeftMatch.begin(), F.mvRightToLeftMatch.end()));
  d.floats(tag + "bounds", {Frame::mnMinX, Frame::mnMinY, Frame::mnMaxX, Frame::mnMaxY});
  d.floats(tag + "sf", F.mvScaleFactors);
  std::vector<int32_t> ids, obs;
  for (MapPoint* p : F.mvpMapPoints) { ids.push_back((int32_t)mp_id(p)); obs.push_back(p ? p->Observations() : -1); }
  d.ints(tag + "held_id", ids);
  d.ints(tag + "held_obs", obs);
}

void dump_pool(Dump& d, const std::string& tag, const std::vector<MapPoint*>& pts) {
  std::vector<unsigned char> pool(pts.size() * 32, 0);
  std::vector<int32_t> ids;
  for (size_t i = 0; i < pts.size(); i++) {
    if (pts[i]) std::memcpy(&pool[i * 32], pts[i]->mDescriptor.ptr<unsigned char>(), 32);
    ids.push_back((int32_t)mp_id(pts[i]));
  }
  d.bytes(tag + "pdesc", pool.data(), pool.size());
  d.ints(tag + "point_id", ids);
}

void result(Dump& d, const std::string& tag, int ret, const Frame& F) {
  d.ints(tag + "ret", {ret});
  std::vector<int32_t> ids;
  for (MapPoint* p : F.mvpMapPoints) ids.push_back((int32_t)mp_id(p));
  d.ints(tag + "mvpMapPoints", ids);
}

// proj_mp_rig: matcher_world.cpp:66-85, variant 2
void local_scenario(Dump& d, const World& w) {
  Scene s(w, false);
  Frame F;
  s.make_rig_frame(F, 2, 3, s.pose(4));
  s.make_points(s.mps, 0, s.pose(0), 0, 0);
  set_track_fields(s, F, s.mps, true);
  prebind(s, F, 11, 30);
  const std::string tag = "local.";
  dump_frame(d, tag, w, F);
  std::vector<MapPoint*> vp;
  for (MapPoint& m : s.mps) vp.push_back(&m);
  dump_pool(d, tag, vp);
  // the rows: isBad() is folded into both flags (the far-point test is off in this call: bFarPoints = false)
  std::vector<float> fl;
  std::vector<int32_t> in;
  for (MapPoint* m : vp) {
    const bool bad = m->isBad();
    fl.insert(fl.end(), {m->mTrackProjX, m->mTrackProjY, m->mTrackViewCos, m->mTrackProjXR, m->mTrackProjYR, m->mTrackViewCosR});
    in.insert(in.end(), {m->mnTrackScaleLevel, m->mnTrackScaleLevelR, m->Observations(), m->mbTrackInView && !bad, m->mbTrackInViewR && !bad});
  }
  d.floats(tag + "rows_f", fl);   // 6 a point
  d.ints(tag + "rows_i", in);     // 5 a point
  d.floats(tag + "call", {3.0f, 0.8f});   // th, mfNNratio
  ORBmatcher matcher(0.8);
  const int ret = matcher.SearchByProjection(F, vp, 3, false, 50.0f);
  result(d, tag + "adapter.", ret, F);
}

// proj_last_rig: matcher_world.cpp:89-121, variant 4, with the scenario's tz or another
void last_scenario(Dump& d, const World& w, const std::string& tag, float tz) {
  Scene s(w, false);
  Frame Last, Cur;
  s.make_rig_frame(Last, 0, 1, s.pose(0));
  s.make_rig_frame(Cur, 2, 3, s.pose(4, 0.01f, 0.005f, tz));
  s.make_points(s.mps, 0, s.pose(0), 0, 0);
  Sophus::SE3f Trw = Last.GetRelativePoseTrl() * Last.GetPose();
  s.make_points(s.mpsB, 1, Trw, 100000, 3);
  for (int i = 0; i < Last.N; i++) {
    MapPoint* p = i < (int)s.mps.size() ? &s.mps[i] : &s.mpsB[i - (int)s.mps.size()];
    if (H(i, 40) % 6 != 0) Last.mvpMapPoints[i] = p;
    Last.mvbOutlier[i] = H(i, 41) % 10 == 0;
  }
  prebind(s, Cur, 13, 42);
  dump_frame(d, tag, w, Cur);
  dump_pool(d, tag, Last.mvpMapPoints);
  // the caller's part of :1686-1733 and :1795-1796
  const float th = 15.f;
  const Sophus::SE3f Tcw = Cur.GetPose();
  const Eigen::Vector3f twc = Tcw.inverse().translation();
  const Sophus::SE3f Tlw = Last.GetPose();
  const Eigen::Vector3f tlc = Tlw * twc;
  const bool bForward = tlc(2) > Cur.mb, bBackward = -tlc(2) > Cur.mb;   // bMono = false
  std::vector<float> fl;
  std::vector<int32_t> in;
  for (int i = 0; i < Last.N; i++) {
    MapPoint* pMP = Last.mvpMapPoints[i];
    float u = 0, v = 0, ur = 0, vr = 0, angle = 0;
    int octave = 0, obs = 0, valid = 0;
    if (pMP && !Last.mvbOutlier[i]) {
      Eigen::Vector3f x3Dw = pMP->GetWorldPos();
      Eigen::Vector3f x3Dc = Tcw * x3Dw;
      const float invzc = 1.0 / x3Dc(2);
      Eigen::Vector2f uv = Cur.mpCamera->project(x3Dc);
      valid = !(invzc < 0) && !(uv(0) < Cur.mnMinX || uv(0) > Cur.mnMaxX) && !(uv(1) < Cur.mnMinY || uv(1) > Cur.mnMaxY);
      Eigen::Vector3f x3Dr = Cur.GetRelativePoseTrl() * x3Dc;
      Eigen::Vector2f uvr = Cur.mpCamera->project(x3Dr);   // :1796 projects with mpCamera
      const cv::KeyPoint& kp = i < Last.Nleft ? Last.mvKeys[i] : Last.mvKeysRight[i - Last.Nleft];
      u = uv(0); v = uv(1); ur = uvr(0); vr = uvr(1); angle = kp.angle; octave = kp.octave; obs = pMP->Observations();
    }
    fl.insert(fl.end(), {u, v, ur, vr, angle});
    in.insert(in.end(), {octave, obs, valid});
  }
  d.floats(tag + "rows_f", fl);   // 5 a point
  d.ints(tag + "rows_i", in);     // 3 a point
  d.floats(tag + "call", {th});
  d.ints(tag + "direction", {bForward ? 1 : bBackward ? 2 : 0});
  ORBmatcher matcher(0.9, true);
  const int ret = matcher.SearchByProjection(Cur, Last, th, false);
  result(d, tag + "adapter.", ret, Cur);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: rig_batch_dump <world.bin> <out.bin>\n"); return 2; }
  World w;
  if (!load_world(argv[1], w) || w.views.size() < 4) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  Dump d{std::fopen(argv[2], "wb")};
  if (!d.f) return 2;
  local_scenario(d, w);
  last_scenario(d, w, "last.", 0.004f);
  last_scenario(d, w, "forward.", -0.3f);
  last_scenario(d, w, "backward.", 0.3f);
  std::fclose(d.f);
  return 0;
}
