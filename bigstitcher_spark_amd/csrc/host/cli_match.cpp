/* `match-interestpoints` — drop-in for the reference's
 * SparkGeometricDescriptorMatching CLI (flag surface:
 * SparkGeometricDescriptorMatching.java:84-156 + AbstractRegistration.java:
 * 62-78; defaults :168-189). Built: -m PRECISE_TRANSLATION, no grouping,
 * same-label matching, timepoints individually. Per view pair the host
 * reads both point lists from interestpoints.n5, maps them to world
 * coordinates with the current registrations, calls libbigstitch's
 * bs_match_descriptors (the RGLDMPairwise replacement, :594-604), runs
 * bs_ransac on the candidates' world coordinates (:564-621 with the models
 * of AbstractRegistration.java:110-140), and stores the inliers as
 * corresponding interest points of both views ([PIN-IPCORR], bs_ipio.h;
 * reference :517-545).
 *
 * Refused with a message and exit 2, never guessed at: -m FAST_ROTATION /
 * FAST_TRANSLATION / ICP, --groupIllums / --groupChannels / --groupTiles /
 * --splitTimepoints, --matchAcrossLabels, -rmc, -rtp other than
 * TIMEPOINTS_INDIVIDUALLY, -ipfr OVERLAPPING_ONLY. */
#include <cfloat>
#include <cstdio>
#include <set>

#include "../../../include/bigstitch.h"
#include "bs_cli_util.h"
#include "bs_ipio.h"
#include "bs_n5.h"
#include "bs_spimdata.h"

namespace {

int model_id(const std::string &s, bool regularizer) {
  if (s == "TRANSLATION") return BS_MODEL_TRANSLATION;
  if (s == "RIGID") return BS_MODEL_RIGID;
  if (s == "AFFINE") return BS_MODEL_AFFINE;
  if (regularizer && s == "NONE") return BS_MODEL_NONE;
  if (regularizer && s == "IDENTITY") return BS_MODEL_IDENTITY;
  return -100;
}

struct ViewPts {
  std::vector<uint64_t> ids;
  std::vector<double> world; /* 3 per point */
};

}  // namespace

int main(int argc, char **argv) {
  bscli::Args args;
  std::map<std::string, std::string> alias = {
      {"-x", "--xml"},
      {"-l", "--label"},
      {"-m", "--method"},
      {"-s", "--significance"},
      {"-sr", "--searchRadius"},
      {"-r", "--redundancy"},
      {"-n", "--numNeighbors"},
      {"-ipfr", "--interestpointsForReg"},
      {"-vr", "--viewReg"},
      {"-rit", "--ransacIterations"},
      {"-rme", "--ransacMaxError"},
      {"-rmir", "--ransacMinInlierRatio"},
      {"-rmni", "--ransacMinNumInliers"},
      {"-rmc", "--ransacMultiConsensus"},
      {"-rtp", "--registrationTP"},
      {"-tm", "--transformationModel"},
      {"-rm", "--regularizationModel"},
      {"-ime", "--icpMaxError"},
      {"-iit", "--icpIterations"},
      {"-vi", "--vi"}};
  const char *usage =
      "usage: match-interestpoints -x dataset.xml -l label [-l label ..] "
      "-m PRECISE_TRANSLATION [-s 3.0] [-sr radius] [-r 1] [-n 3] "
      "[--clearCorrespondences] [-vr OVERLAPPING_ONLY|ALL_AGAINST_ALL] "
      "[-rit 10000] [-rme 5.0] [-rmir 0.1] [-rmni 12] "
      "[-tm TRANSLATION|RIGID|AFFINE] [-rm NONE|IDENTITY|TRANSLATION|RIGID|"
      "AFFINE] [--lambda 0.1] [-vi 'tp,setup' ... | --angleId/--tileId/"
      "--channelId/--illuminationId/--timepointId '0,1,..'] [--device N] "
      "[--dryRun]\n";
  if (!args.parse(argc, argv, alias,
                  {"clearCorrespondences", "dryRun", "matchAcrossLabels",
                   "groupIllums", "groupChannels", "groupTiles",
                   "splitTimepoints", "ransacMultiConsensus",
                   "icpUseRANSAC"})) {
    fputs(usage, stderr);
    return 2;
  }
  for (const char *f : {"xml", "label", "method"})
    if (!args.has(f)) {
      fprintf(stderr, "error: missing required option --%s\n", f);
      fputs(usage, stderr);
      return 2;
    }
  /* refused before anything else happens (no XML read, no GPU call) */
  const std::string method = args.get("method");
  if (method == "FAST_ROTATION" || method == "FAST_TRANSLATION" ||
      method == "ICP") {
    fprintf(stderr,
            "error: -m %s is not supported by this build "
            "(PRECISE_TRANSLATION only)\n",
            method.c_str());
    return 2;
  }
  if (method != "PRECISE_TRANSLATION") {
    fprintf(stderr, "error: unknown --method %s\n", method.c_str());
    return 2;
  }
  for (const char *f : {"groupIllums", "groupChannels", "groupTiles",
                        "splitTimepoints", "matchAcrossLabels",
                        "ransacMultiConsensus", "interestPointMergeDistance",
                        "icpMaxError", "icpIterations", "icpUseRANSAC",
                        "referenceTP", "rangeTP"})
    if (args.has(f)) {
      fprintf(stderr, "error: --%s is not supported by this build\n", f);
      return 2;
    }
  if (args.get("registrationTP", "TIMEPOINTS_INDIVIDUALLY") !=
      "TIMEPOINTS_INDIVIDUALLY") {
    fprintf(stderr,
            "error: -rtp %s is not supported by this build "
            "(TIMEPOINTS_INDIVIDUALLY only)\n",
            args.get("registrationTP").c_str());
    return 2;
  }
  if (args.get("interestpointsForReg", "ALL") != "ALL") {
    fprintf(stderr,
            "error: -ipfr %s is not supported by this build (ALL only)\n",
            args.get("interestpointsForReg").c_str());
    return 2;
  }
  const std::string viewReg = args.get("viewReg", "OVERLAPPING_ONLY");
  if (viewReg != "OVERLAPPING_ONLY" && viewReg != "ALL_AGAINST_ALL") {
    fprintf(stderr, "error: unknown --viewReg %s\n", viewReg.c_str());
    return 2;
  }
  bs_ransac_params rp{};
  rp.model = model_id(args.get("transformationModel", "AFFINE"), false);
  rp.regularizer = model_id(args.get("regularizationModel", "RIGID"), true);
  if (rp.model == -100 || rp.regularizer == -100) {
    fprintf(stderr, "error: unknown -tm / -rm model\n");
    return 2;
  }
  rp.lambda = args.getd("lambda", 0.1);
  rp.max_epsilon = args.getd("ransacMaxError", 5.0);
  rp.min_inlier_ratio = args.getd("ransacMinInlierRatio", 0.1);
  rp.min_num_inliers = (int32_t)args.getl("ransacMinNumInliers", 12);
  rp.iterations = (int32_t)args.getl("ransacIterations", 10000);
  bs_match_params mp{};
  mp.num_neighbors = (int32_t)args.getl("numNeighbors", 3);
  mp.redundancy = (int32_t)args.getl("redundancy", 1);
  mp.ratio_of_distance = (float)args.getd("significance", 3.0);
  mp.difference_threshold = FLT_MAX;
  mp.limit_search_radius = args.has("searchRadius") ? 1 : 0;
  mp.search_radius = args.getd("searchRadius", 0.0);
  const std::vector<std::string> labels = args.getall("label");
  const bool clear = args.has("clearCorrespondences");
  const bool dryRun = args.has("dryRun");

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
  /* every selected view must carry every label (reference :643-647) */
  std::set<std::pair<bssd::ViewId, std::string>> have;
  for (auto &e : sd.interest_points())
    have.insert({{e.timepoint, e.setup}, e.label});
  for (auto &v : selected)
    for (auto &l : labels)
      if (!have.count({v, l})) {
        fprintf(stderr,
                "error: view (%d,%d) has no interest points with label '%s'\n",
                v.first, v.second, l.c_str());
        return 1;
      }
  const std::string ipn5 = bsip::ipn5_path(args.get("xml"));
  bsn5::Container c(ipn5);
  if (!c.exists()) {
    fprintf(stderr, "error: %s does not exist\n", ipn5.c_str());
    return 1;
  }

  /* view pairs: same timepoint, A < B */
  std::vector<std::pair<bssd::ViewId, bssd::ViewId>> pairs;
  for (size_t i = 0; i < selected.size(); ++i)
    for (size_t j = i + 1; j < selected.size(); ++j) {
      const auto &A = selected[i], &B = selected[j];
      if (A.first != B.first) continue;
      if (viewReg == "OVERLAPPING_ONLY") {
        const bssd::ViewSetup *sa = sd.setup(A.second), *sb = sd.setup(B.second);
        if (!sa || !sb) continue;
        double loA[3], hiA[3], loB[3], hiB[3];
        bscli::tbbox(sd.regs.at(A), sa->dims, loA, hiA);
        bscli::tbbox(sd.regs.at(B), sb->dims, loB, hiB);
        bool ovl = true;
        for (int d = 0; d < 3; ++d)
          if (std::min(hiA[d], hiB[d]) <= std::max(loA[d], loB[d])) ovl = false;
        if (!ovl) continue;
      }
      pairs.push_back({A, B});
    }
  printf("match-interestpoints: %zu views, %zu labels, %zu pairs (%s), "
         "n=%d r=%d significance=%g%s\n",
         selected.size(), labels.size(), pairs.size(), viewReg.c_str(),
         mp.num_neighbors, mp.redundancy, (double)mp.ratio_of_distance,
         mp.limit_search_radius ? " with search radius" : "");

  bs_ctx *ctx = nullptr;
  if (bs_ctx_create(&ctx, (int)args.getl("device", 0)) != BS_OK) {
    fprintf(stderr, "error: %s\n", bs_last_error(nullptr));
    return 1;
  }

  for (auto &label : labels) {
    /* points of every selected view in world coordinates */
    std::map<bssd::ViewId, ViewPts> pts;
    for (auto &v : selected) {
      ViewPts vp;
      std::vector<double> loc;
      const std::string group =
          bssd::SpimData::interest_point_group(v.first, v.second, label);
      if (!bsip::read_points(c, group, &vp.ids, &loc)) {
        fprintf(stderr, "error: cannot read %s/%s\n", ipn5.c_str(),
                group.c_str());
        return 1;
      }
      const auto &m = sd.regs.at(v);
      vp.world.resize(loc.size());
      for (size_t i = 0; i < vp.ids.size(); ++i)
        for (int r = 0; r < 3; ++r)
          vp.world[3 * i + r] = m[4 * r] * loc[3 * i] +
                                m[4 * r + 1] * loc[3 * i + 1] +
                                m[4 * r + 2] * loc[3 * i + 2] + m[4 * r + 3];
      pts[v] = std::move(vp);
    }
    std::map<bssd::ViewId, std::vector<bsip::Corr>> fresh;
    for (auto &pr : pairs) {
      const ViewPts &A = pts[pr.first], &B = pts[pr.second];
      size_t n = 0;
      int rc = bs_match_descriptors(ctx, A.world.data(), A.ids.size(),
                                    B.world.data(), B.ids.size(), &mp, nullptr,
                                    0, &n);
      std::vector<bs_match_candidate> cand(n);
      if (rc == BS_OK && n)
        rc = bs_match_descriptors(ctx, A.world.data(), A.ids.size(),
                                  B.world.data(), B.ids.size(), &mp,
                                  cand.data(), cand.size(), &n);
      if (rc != BS_OK || n != cand.size()) {
        fprintf(stderr, "matching failed for (%d,%d)-(%d,%d): rc=%d %s\n",
                pr.first.first, pr.first.second, pr.second.first,
                pr.second.second, rc, bs_last_error(ctx));
        return rc == BS_EUNSUP ? 2 : 1;
      }
      std::vector<double> pa(3 * n), pb(3 * n);
      for (size_t i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d) {
          pa[3 * i + d] = A.world[3 * (size_t)cand[i].a + d];
          pb[3 * i + d] = B.world[3 * (size_t)cand[i].b + d];
        }
      std::vector<uint8_t> inl(n);
      double M[12];
      size_t nin = 0;
      if (bs_ransac(pa.data(), pb.data(), n, &rp, inl.data(), M, &nin) !=
          BS_OK) {
        fprintf(stderr, "error: bad RANSAC parameters\n");
        return 2;
      }
      printf("pair (%d,%d)-(%d,%d) label '%s': %zu candidates, %zu inliers, "
             "translation (%.4f, %.4f, %.4f)\n",
             pr.first.first, pr.first.second, pr.second.first,
             pr.second.second, label.c_str(), n, nin, M[3], M[7], M[11]);
      for (size_t i = 0; i < n; ++i) {
        if (!inl[i]) continue;
        bsip::Corr ka, kb;
        ka.id = A.ids[cand[i].a];
        ka.other_id = B.ids[cand[i].b];
        ka.other = pr.second;
        ka.other_label = label;
        kb.id = ka.other_id;
        kb.other_id = ka.id;
        kb.other = pr.first;
        kb.other_label = label;
        fresh[pr.first].push_back(ka);
        fresh[pr.second].push_back(kb);
      }
    }
    if (dryRun) continue;
    /* processed views: existing entries kept (or cleared), new appended */
    for (auto &v : selected) {
      const std::string group =
          bssd::SpimData::interest_point_group(v.first, v.second, label);
      std::vector<bsip::Corr> list;
      if (!clear && !bsip::read_corrs(c, group, &list)) {
        fprintf(stderr, "error: inconsistent correspondences in %s/%s\n",
                ipn5.c_str(), group.c_str());
        return 1;
      }
      auto it = fresh.find(v);
      if (it != fresh.end())
        list.insert(list.end(), it->second.begin(), it->second.end());
      if (!bsip::write_corrs(c, group, list)) {
        fprintf(stderr, "error: cannot write %s/%s\n", ipn5.c_str(),
                group.c_str());
        return 1;
      }
    }
  }
  bs_ctx_destroy(ctx);
  if (dryRun)
    printf("--dryRun: nothing written\n");
  else
    printf("saved correspondences of %zu views to %s\n", selected.size(),
           ipn5.c_str());
  return 0;
}
