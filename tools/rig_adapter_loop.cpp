// BENCH INFRASTRUCTURE: the per-frame loop through the drop-in adapter's two-camera rig path (include/ORBmatcher.h +
// csrc/ref_adapter/ORBmatcher.cc over liborbx.so) on the inputs of tools/rigmatch_times.py: leg (a) of profiles/rigmatch_times_r24.txt.
// For every item it builds the rig Frame from the tool's arrays through tests/support/world_scene.h (pinhole cameras, identity pose, a
// pure-baseline Trl), the map points of SearchLocalPoints with the tool's track fields, and a last frame whose points lie at depth kZ
// behind the tool's (u, v); then, as Tracking does on a new frame, SearchByProjection(Cur, Last, th, false) first (the frame becomes
// resident in this call) and SearchByProjection(Cur, map points, th) second, each on the same pre-bound slots.  Only the matcher calls are
// timed (steady_clock).  It writes the rows the LastFrame caller computed (:1686-1733, :1795-1796), so that the batched call runs on the
// same numbers, and both calls' mvpMapPoints as ids, so that the tool can hold the two paths equal.
//
//   rig_adapter_loop <in.bin> <out.bin> <passes>
// Records as tests/support/rig_batch_dump.cpp: {int32 name length, name, int32 kind (0 int32, 1 float32, 2 bytes), int32 count, data}.
#include <map>

#include "world_scene.h"

namespace {

constexpr float kZ = 3.0f;

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

struct LocalRow { float proj_x, proj_y, view_cos; int32_t level; float proj_xr, proj_yr, view_cos_r; int32_t level_r, obs, point, in_view, in_view_r; };
struct LastSpec { float u, v, angle; int32_t octave, obs, point, valid; };   // what the tool asks of a last-frame point

void set_slots(Frame& F, std::vector<MapPoint>& extra, const int32_t* kp_obs) {
  for (int i = 0; i < F.N; i++) {
    extra[i].mnId = 900000 + i;
    extra[i].nObs = kp_obs[i];
    F.mvpMapPoints[i] = kp_obs[i] >= 0 ? &extra[i] : static_cast<MapPoint*>(NULL);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: rig_adapter_loop <in.bin> <out.bin> <passes>\n"); return 2; }
  const auto in = read_records(argv[1]);
  const int passes = std::atoi(argv[3]);
  const int32_t* shape = as<int32_t>(in, "shape");   // items, features a side, points an item, image size
  const int B = shape[0], n = shape[1], npts = shape[2], size = shape[3];
  const float* sf = as<float>(in, "sf");
  const float th_local = as<float>(in, "call")[0], ratio_local = as<float>(in, "call")[1], th_last = as<float>(in, "call")[2], shift = as<float>(in, "call")[3];
  const cv::KeyPoint* kl = as<cv::KeyPoint>(in, "kps_l");
  const cv::KeyPoint* kr = as<cv::KeyPoint>(in, "kps_r");
  const unsigned char *dl = as<unsigned char>(in, "desc_l"), *dr = as<unsigned char>(in, "desc_r"), *pool = as<unsigned char>(in, "pdesc");
  const int32_t *l2r = as<int32_t>(in, "l2r"), *r2l = as<int32_t>(in, "r2l"), *kp_obs = as<int32_t>(in, "kp_obs");
  const LocalRow* mp = as<LocalRow>(in, "mp");
  const LastSpec* spec = as<LastSpec>(in, "last_spec");

  std::vector<float> rows_f((size_t)B * npts * 5, 0.f), ms_last, ms_local;
  std::vector<int32_t> rows_i((size_t)B * npts * 3, 0), ids_last((size_t)B * 2 * n, -1), ids_local((size_t)B * 2 * n, -1), ret_last(B, 0), ret_local(B, 0);
  for (int pass = 0; pass < passes; pass++) {
    double t_last = 0, t_local = 0;
    for (int b = 0; b < B; b++) {
      World w;
      w.rows = size; w.cols = size; w.nlevels = 8;
      w.scale.assign(sf, sf + 8); w.sigma2.resize(8); w.inv_sigma2.resize(8);
      for (int l = 0; l < 8; l++) { w.sigma2[l] = sf[l] * sf[l]; w.inv_sigma2[l] = 1.f / w.sigma2[l]; }
      w.logScaleFactor = std::log(1.2f);
      w.views.resize(2);
      for (int c = 0; c < 2; c++) {
        View& V = w.views[c];
        V.n = n;
        V.kps.assign((c ? kr : kl) + (size_t)b * n, (c ? kr : kl) + (size_t)(b + 1) * n);
        V.desc = cv::Mat(n, 32, CV_8U);
        std::memcpy(V.desc.data, (c ? dr : dl) + (size_t)b * n * 32, (size_t)n * 32);
      }
      Scene s(w, false);
      Frame Cur, Last;
      s.make_rig_frame(Cur, 0, 1, s.pose(0));
      Cur.mvLeftToRightMatch.assign(l2r + (size_t)b * n, l2r + (size_t)(b + 1) * n);
      Cur.mvRightToLeftMatch.assign(r2l + (size_t)b * n, r2l + (size_t)(b + 1) * n);
      Cur.mpCamera = &s.cams.pinL; Cur.mpCamera2 = &s.cams.pinR;
      Cur.mTrl = Sophus::SE3f(rot_yx(0.f, 0.f), Eigen::Vector3f(-shift * kZ / s.cams.pinL.fx, 0.f, 0.f));   // u_r = u - shift at depth kZ
      const int32_t* obs_row = kp_obs + (size_t)b * 2 * n;
      std::vector<MapPoint> extra(Cur.N), local(npts), lastp(npts);
      // ---- the last frame: point q behind (u, v) of the current (= the last) camera
      s.fill_common(Last);
      Last.mnId = Scene::nextFrameId++;
      Last.N = npts; Last.Nleft = -1; Last.Nright = -1;
      Last.mvKeys.resize(npts); Last.mvKeysUn.resize(npts);
      Last.mvpMapPoints.assign(npts, static_cast<MapPoint*>(NULL));
      Last.mvbOutlier.assign(npts, false);
      Last.mTcw = s.pose(0);
      for (int q = 0; q < npts; q++) {
        const LastSpec& p = spec[(size_t)b * npts + q];
        MapPoint& m = lastp[q];
        m.mnId = q; m.nObs = p.obs;
        m.mWorldPos = Eigen::Vector3f((p.u - s.cams.pinL.cx) / s.cams.pinL.fx * kZ, (p.v - s.cams.pinL.cy) / s.cams.pinL.fy * kZ, kZ);
        m.mDescriptor = cv::Mat(1, 32, CV_8U);
        std::memcpy(m.mDescriptor.data, pool + (size_t)p.point * 32, 32);
        Last.mvKeys[q].angle = p.angle; Last.mvKeys[q].octave = p.octave;
        Last.mvKeysUn[q] = Last.mvKeys[q];
        if (p.valid) Last.mvpMapPoints[q] = &m;
      }
      if (pass == 0) {   // the caller's rows, as tests/support/rig_batch_dump.cpp computes them
        const Sophus::SE3f Tcw = Cur.GetPose();
        for (int q = 0; q < npts; q++) {
          MapPoint* pMP = Last.mvpMapPoints[q];
          if (!pMP) continue;
          Eigen::Vector3f x3Dc = Tcw * pMP->GetWorldPos();
          const float invzc = 1.0 / x3Dc(2);
          Eigen::Vector2f uv = Cur.mpCamera->project(x3Dc);
          Eigen::Vector3f x3Dr = Cur.GetRelativePoseTrl() * x3Dc;
          Eigen::Vector2f uvr = Cur.mpCamera->project(x3Dr);
          float* f = &rows_f[((size_t)b * npts + q) * 5];
          int32_t* i = &rows_i[((size_t)b * npts + q) * 3];
          f[0] = uv(0); f[1] = uv(1); f[2] = uvr(0); f[3] = uvr(1); f[4] = Last.mvKeys[q].angle;
          i[0] = Last.mvKeys[q].octave; i[1] = pMP->Observations();
          i[2] = !(invzc < 0) && !(uv(0) < Cur.mnMinX || uv(0) > Cur.mnMaxX) && !(uv(1) < Cur.mnMinY || uv(1) > Cur.mnMaxY);
        }
      }
      // ---- the local map: the tool's track fields
      std::vector<MapPoint*> vp;
      for (int q = 0; q < npts; q++) {
        const LocalRow& p = mp[(size_t)b * npts + q];
        MapPoint& m = local[q];
        m.mnId = q; m.nObs = p.obs;
        m.mbTrackInView = p.in_view != 0; m.mbTrackInViewR = p.in_view_r != 0;
        m.mTrackProjX = p.proj_x; m.mTrackProjY = p.proj_y; m.mTrackViewCos = p.view_cos; m.mnTrackScaleLevel = p.level;
        m.mTrackProjXR = p.proj_xr; m.mTrackProjYR = p.proj_yr; m.mTrackViewCosR = p.view_cos_r; m.mnTrackScaleLevelR = p.level_r;
        m.mDescriptor = cv::Mat(1, 32, CV_8U);
        std::memcpy(m.mDescriptor.data, pool + (size_t)p.point * 32, 32);
        vp.push_back(&m);
      }
      // ---- Tracking's order on a new frame: TrackWithMotionModel's search, then SearchLocalPoints; the same slots before each
      set_slots(Cur, extra, obs_row);
      ORBmatcher m_last(0.9, true), m_local(ratio_local);
      auto t0 = std::chrono::steady_clock::now();
      const int r1 = m_last.SearchByProjection(Cur, Last, th_last, false);
      auto t1 = std::chrono::steady_clock::now();
      t_last += std::chrono::duration<double, std::milli>(t1 - t0).count();
      if (pass == 0) {
        ret_last[b] = r1;
        for (int i = 0; i < Cur.N; i++) ids_last[(size_t)b * 2 * n + i] = (int32_t)mp_id(Cur.mvpMapPoints[i]);
      }
      set_slots(Cur, extra, obs_row);
      t0 = std::chrono::steady_clock::now();
      const int r2 = m_local.SearchByProjection(Cur, vp, th_local, false, 50.0f);
      t1 = std::chrono::steady_clock::now();
      t_local += std::chrono::duration<double, std::milli>(t1 - t0).count();
      if (pass == 0) {
        ret_local[b] = r2;
        for (int i = 0; i < Cur.N; i++) ids_local[(size_t)b * 2 * n + i] = (int32_t)mp_id(Cur.mvpMapPoints[i]);
      }
    }
    ms_last.push_back((float)t_last); ms_local.push_back((float)t_local);
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  write_rec(o, "rows_f", 1, rows_f.data(), rows_f.size());
  write_rec(o, "rows_i", 0, rows_i.data(), rows_i.size());
  write_rec(o, "ids_last", 0, ids_last.data(), ids_last.size());
  write_rec(o, "ids_local", 0, ids_local.data(), ids_local.size());
  write_rec(o, "ret_last", 0, ret_last.data(), ret_last.size());
  write_rec(o, "ret_local", 0, ret_local.data(), ret_local.size());
  write_rec(o, "ms_last", 1, ms_last.data(), ms_last.size());
  write_rec(o, "ms_local", 1, ms_local.data(), ms_local.size());
  std::fclose(o);
  return 0;
}
