/* `match-intensities` — drop-in for the reference's SparkIntensityMatching
 * CLI (flag surface: SparkIntensityMatching.java:42-77 plus the view
 * selection of AbstractSelectableViews). Every pair of selected views whose
 * transformed bounding boxes intersect (:146-161) is one work unit: the host
 * opens both views at the pyramid level the fusion CLI would pick for the
 * render grid's sampling step ([PIN-MIP] folded into the affine), and
 * libbigstitch's bs_intensity_match_pair (the IntensityCorrection.matchRansac
 * replacement, :173-174) returns the accepted coefficient-cell buckets, which
 * are stored in the [PIN-INTMATCH-IO] container at -o (bs_intio.h).
 *
 * Views stay resident across pairs; a view is released after its last pair,
 * and when the next pair would not fit the free-HBM budget the least
 * recently used views are evicted first (they are read again if needed).
 *
 * Not built, refused with exit 2: --method HISTOGRAM and a --maxTrust other
 * than 3 ([PIN-INT-TRUST]: the median-cost trim is not applied). */
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <map>
#include <set>

#include "../../../include/bigstitch.h"
#include "bs_cli_util.h"
#include "bs_imgio.h"
#include "bs_intio.h"
#include "bs_mip.h"
#include "bs_n5.h"
#include "bs_spimdata.h"

namespace {

struct ViewPlan {
  bssd::ViewId id;
  int level = 0;
  bscli::M34 affine{};            /* level-local -> world */
  long long dims[3] = {0, 0, 0};  /* level dims */
  double lo[3], hi[3];            /* world bbox */
  size_t bytes = 0;
};

std::string strip_file_uri(const std::string &s) {
  return s.rfind("file:", 0) == 0 ? s.substr(5) : s;
}

}  // namespace

int main(int argc, char **argv) {
  bscli::Args args;
  std::map<std::string, std::string> alias = {
      {"-x", "--xml"}, {"-o", "--outputPath"}, {"-vi", "--vi"}};
  const char *usage =
      "usage: match-intensities -x dataset.xml -o matches.n5 "
      "[--numCoefficients 8,8,8] [--renderScale 0.25] [--minThreshold 1] "
      "[--maxThreshold T] [--minNumCandidates 1000] [--method RANSAC] "
      "[--numIterations 1000] [--maxEpsilon 5.1] [--minInlierRatio 0.1] "
      "[--minNumInliers 10] [--maxTrust 3] [-vi 'tp,setup' ... | --angleId/"
      "--tileId/--channelId/--illuminationId/--timepointId '0,1,..'] "
      "[--device N] [--dryRun]\n";
  if (!args.parse(argc, argv, alias, {"dryRun", "localSparkBindAddress"})) {
    fputs(usage, stderr);
    return 2;
  }
  /* refused before anything else happens (no XML read, no GPU call) */
  if (args.get("method", "RANSAC") != "RANSAC") {
    fprintf(stderr, "error: --method %s is not built (RANSAC only)\n",
            args.get("method").c_str());
    return 2;
  }
  if (args.getd("maxTrust", 3.0) != 3.0) {
    fprintf(stderr, "error: --maxTrust other than 3 is not built (the "
                    "median-cost trim is not applied)\n");
    return 2;
  }
  for (const char *f : {"xml", "outputPath"})
    if (!args.has(f)) {
      fprintf(stderr, "error: missing required option --%s\n", f);
      fputs(usage, stderr);
      return 2;
    }
  for (const char *f : {"s3Region", "localSparkBindAddress"})
    if (args.has(f))
      fprintf(stderr, "note: --%s accepted for compatibility (no-op in "
                      "this build)\n", f);
  bs_intensity_params prm{};
  prm.render_scale = args.getd("renderScale", 0.25);
  auto nc = bscli::parse_ints(args.get("numCoefficients", "8,8,8"));
  if (nc.size() != 3 || nc[0] < 1 || nc[1] < 1 || nc[2] < 1) {
    fprintf(stderr, "error: --numCoefficients needs three counts >= 1\n");
    return 2;
  }
  for (int d = 0; d < 3; ++d) prm.coefficients[d] = (int32_t)nc[d];
  prm.min_num_candidates = (int32_t)args.getl("minNumCandidates", 1000);
  prm.min_threshold = args.getd("minThreshold", 1.0);
  prm.max_threshold = args.has("maxThreshold") ? args.getd("maxThreshold", 0)
                                               : std::nan("");
  prm.iterations = (int32_t)args.getl("numIterations", 1000);
  prm.min_num_inliers = (int32_t)args.getl("minNumInliers", 10);
  prm.max_epsilon = args.getd("maxEpsilon", 0.02 * 255);
  prm.min_inlier_ratio = args.getd("minInlierRatio", 0.1);
  if (!(prm.render_scale > 0.0 && prm.render_scale <= 1.0) ||
      prm.iterations < 1 || prm.iterations > 4096) {
    fprintf(stderr, "error: need --renderScale in (0, 1] and "
                    "--numIterations in 1..4096\n");
    return 2;
  }

  bssd::SpimData sd;
  std::string err;
  if (!sd.load(args.get("xml"), &err)) {
    fprintf(stderr, "error: %s\n", err.c_str());
    return 1;
  }
  std::vector<bssd::ViewId> selected;
  if (!bssd::select_views(sd, args.getall("vi"), args.get("angleId"),
                          args.get("tileId"), args.get("illuminationId"),
                          args.get("channelId"), args.get("timepointId"),
                          &selected, &err)) {
    fprintf(stderr, "error: %s\n", err.c_str());
    return 1;
  }

  /* per view: level by the fusion CLI's sampling-step rule, applied to the
   * view -> render-grid transform, and the level folded into the affine */
  bsimg::Input input(sd);
  std::vector<ViewPlan> views;
  for (auto &vid : selected) {
    auto r = sd.regs.find(vid);
    if (r == sd.regs.end()) continue;
    ViewPlan v;
    v.id = vid;
    for (int i = 0; i < 12; ++i) v.affine[i] = r->second[i];
    auto levels = input.read_levels(vid.second, vid.first);
    bscli::M34 togrid = v.affine;
    for (auto &e : togrid) e *= prm.render_scale;
    const int lvi = bscli::pick_level_for_transform(togrid, levels);
    long long lf[3] = {1, 1, 1};
    if (lvi > 0 && lvi < (int)levels.size()) {
      for (int d = 0; d < 3; ++d) lf[d] = levels[lvi].f[d];
      for (int rr = 0; rr < 3; ++rr) { /* [PIN-MIP] */
        double off = 0;
        for (int cc = 0; cc < 3; ++cc) {
          off += v.affine[rr * 4 + cc] * 0.5 * (double)(lf[cc] - 1);
          v.affine[rr * 4 + cc] *= (double)lf[cc];
        }
        v.affine[rr * 4 + 3] += off;
      }
      v.level = levels[lvi].level;
    }
    const bssd::ViewSetup *s = sd.setup(vid.second);
    if (lvi >= 0 && lvi < (int)levels.size() && levels[lvi].dims.size() == 3) {
      for (int d = 0; d < 3; ++d) v.dims[d] = levels[lvi].dims[d];
    } else if (s) {
      for (int d = 0; d < 3; ++d) v.dims[d] = (s->dims[d] + lf[d] - 1) / lf[d];
    }
    if (v.dims[0] < 1 || v.dims[1] < 1 || v.dims[2] < 1) {
      fprintf(stderr, "error: unknown dimensions of view (%d,%d)\n",
              vid.first, vid.second);
      return 1;
    }
    bscli::tbbox(v.affine, v.dims, v.lo, v.hi);
    v.bytes = (size_t)v.dims[0] * v.dims[1] * v.dims[2] * 2;
    views.push_back(v);
  }
  if (views.empty()) {
    fprintf(stderr, "error: no views selected\n");
    return 1;
  }
  /* pairs: bounding boxes intersect (reference :146-161) */
  std::vector<std::pair<int, int>> pairs;
  for (size_t i = 0; i < views.size(); ++i)
    for (size_t j = i + 1; j < views.size(); ++j) {
      bool hit = true;
      for (int d = 0; d < 3; ++d)
        hit = hit && std::max(views[i].lo[d], views[j].lo[d]) <=
                         std::min(views[i].hi[d], views[j].hi[d]);
      if (hit) pairs.push_back({(int)i, (int)j});
    }
  printf("match-intensities: %zu views, %zu overlapping pairs, coefficients "
         "%d,%d,%d, renderScale %g, %d iterations\n",
         views.size(), pairs.size(), prm.coefficients[0], prm.coefficients[1],
         prm.coefficients[2], prm.render_scale, prm.iterations);
  if (args.has("dryRun")) {
    printf("--dryRun: nothing written\n");
    return 0;
  }

  bsn5::Container out(strip_file_uri(args.get("outputPath")));
  if (!out.create() ||
      !bsint_io::write_coefficients_size(out, prm.coefficients)) {
    fprintf(stderr, "error: cannot create %s\n", out.root().c_str());
    return 1;
  }
  bs_ctx *ctx = nullptr;
  if (bs_ctx_create(&ctx, (int)args.getl("device", 0)) != BS_OK) {
    fprintf(stderr, "error: %s\n", bs_last_error(nullptr));
    return 1;
  }
  uint64_t freeb = 0, totb = 0;
  (void)bs_device_mem(ctx, &freeb, &totb);
  size_t budget = freeb > (8UL << 30) ? (size_t)freeb - (4UL << 30)
                                      : (size_t)freeb * 3 / 4;
  if (const char *e = getenv("BS_INTENSITY_BUDGET_MB"))
    budget = (size_t)atoll(e) << 20;
  std::vector<size_t> last_use(views.size(), 0);
  for (size_t k = 0; k < pairs.size(); ++k)
    last_use[pairs[k].first] = last_use[pairs[k].second] = k;
  std::map<int, size_t> resident; /* view index -> pair index of last use */
  size_t resident_bytes = 0, uploads = 0;
  auto release = [&](int vi) {
    (void)bs_view_release(ctx, vi);
    resident_bytes -= views[vi].bytes;
    resident.erase(vi);
  };
  size_t total_buckets = 0;
  for (size_t k = 0; k < pairs.size(); ++k) {
    const int pa = pairs[k].first, pb = pairs[k].second;
    for (int vi : {pa, pb}) {
      if (resident.count(vi)) {
        resident[vi] = k;
        continue;
      }
      /* make room: least recently used first, never this pair's views */
      while (!resident.empty() && resident_bytes + views[vi].bytes > budget) {
        int victim = -1;
        for (auto &kv : resident)
          if (kv.first != pa && kv.first != pb &&
              (victim < 0 || kv.second < resident[victim]))
            victim = kv.first;
        if (victim < 0) break;
        release(victim);
      }
      std::vector<uint16_t> vox;
      std::vector<long long> dims;
      const ViewPlan &v = views[vi];
      if (!input.read_volume_u16(v.id.second, v.id.first, v.level, &vox,
                                 &dims) ||
          dims.size() != 3 || dims[0] != v.dims[0] || dims[1] != v.dims[1] ||
          dims[2] != v.dims[2]) {
        fprintf(stderr, "cannot read view tp=%d setup=%d level %d from %s\n",
                v.id.first, v.id.second, v.level, sd.n5_path.c_str());
        return 1;
      }
      const int64_t d3[3] = {dims[0], dims[1], dims[2]};
      if (bs_view_upload(ctx, vi, vox.data(), d3) != BS_OK) {
        fprintf(stderr, "upload failed: %s\n", bs_last_error(ctx));
        return 1;
      }
      resident[vi] = k;
      resident_bytes += v.bytes;
      ++uploads;
    }
    /* one call is enough unless more buckets come back than guessed */
    size_t n = 0;
    std::vector<bs_intensity_match> m(1024);
    int rc = bs_intensity_match_pair(ctx, pa, views[pa].affine.data(), pb,
                                     views[pb].affine.data(), &prm, m.data(),
                                     m.size(), &n);
    if (rc == BS_OK && n > m.size()) {
      m.resize(n);
      rc = bs_intensity_match_pair(ctx, pa, views[pa].affine.data(), pb,
                                   views[pb].affine.data(), &prm, m.data(),
                                   m.size(), &n);
    }
    if (rc == BS_OK && n <= m.size()) m.resize(n);
    if (rc != BS_OK || n != m.size()) {
      fprintf(stderr, "matching failed for (%d,%d) <> (%d,%d): rc=%d %s\n",
              views[pa].id.first, views[pa].id.second, views[pb].id.first,
              views[pb].id.second, rc, bs_last_error(ctx));
      return 1;
    }
    if (!bsint_io::write_pair(out, views[pa].id, views[pb].id, m)) {
      fprintf(stderr, "error: cannot write %s\n",
              bsint_io::pair_dataset(views[pa].id, views[pb].id).c_str());
      return 1;
    }
    uint64_t inl = 0;
    for (auto &r : m) inl += r.n_inl;
    printf("(%d,%d) <> (%d,%d): levels %d/%d, %zu buckets, %" PRIu64
           " inliers\n",
           views[pa].id.first, views[pa].id.second, views[pb].id.first,
           views[pb].id.second, views[pa].level, views[pb].level, m.size(),
           inl);
    total_buckets += m.size();
    for (int vi : {pa, pb})
      if (last_use[vi] == k && resident.count(vi)) release(vi);
  }
  bs_batch_stats st;
  if (bs_get_stats(ctx, &st) == BS_OK)
    printf("kernels: render %.3f ms, moments %.3f ms, ransac %.3f ms; %zu "
           "view uploads\n",
           st.total_ms[BS_K_INT_RENDER], st.total_ms[BS_K_INT_MOMENTS],
           st.total_ms[BS_K_INT_RANSAC], uploads);
  bs_ctx_destroy(ctx);
  printf("saved %zu buckets of %zu pairs to %s\n", total_buckets, pairs.size(),
         out.root().c_str());
  return 0;
}
