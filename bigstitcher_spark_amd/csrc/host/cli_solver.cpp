/* `solver` — drop-in for the reference's Solver CLI (reference
 * Solver.java; a multi-threaded host tool, not Spark — README.md:220).
 * Consumes the <StitchingResults> links written by `stitching`:
 *   1. drops links whose stored hash no longer matches the current
 *      registrations (Solver.java:404-415 semantics; hash rule
 *      [PIN-HASH] in bs_spimdata.h),
 *   2. solves the global translation adjustment minimising
 *      sum_links r_link * || (t_B - t_A) - d_link ||^2 with the first (or
 *      --fixedViews) view fixed — the translation case of the
 *      reference's GlobalOpt tile optimisation (Solver.java:301-337;
 *      the mpicbg TranslationModel3D path) as a direct graph-Laplacian
 *      least squares,
 *   3. prepends a "Stitching Transform" translation to each view's
 *      registration chain and saves the XML.
 * d_link: the stored link matrix's translation ws satisfies
 * "B's content appears at +ws relative to where the current
 * registrations place it" is ws = -correction, i.e. the solved
 * adjustment should satisfy t_B - t_A = -ws.
 *
 * -s/--sourcePoints IP (Solver.java:434-670) takes the links from the
 * corresponding interest points `match-interestpoints` stored instead
 * ([PIN-IPCORR], bs_ipio.h): for each view pair A < B and each -l label,
 * A's correspondence list gives d = mean(pA_world - pB_world) over its
 * matches with B, weighted by match count x label weight (-lw); the
 * prepended transform is then named "Interest Point Transform"
 * ([PIN-XML] restatement). Only -tm TRANSLATION is built. Without -s (or
 * with -s STITCHING) nothing changes. */
#include <cmath>
#include <array>
#include <cstdio>
#include <map>
#include <set>

#include "bs_cli_util.h"
#include "bs_ipio.h"
#include "bs_spimdata.h"

int main(int argc, char **argv) {
  bscli::Args args;
  std::map<std::string, std::string> alias = {
      {"-x", "--xml"},           {"-s", "--sourcePoints"},
      {"-l", "--label"},         {"-lw", "--labelweights"},
      {"-tm", "--transformationModel"}};
  if (!args.parse(argc, argv, alias, {"dryRun"}) || !args.has("xml")) {
    fprintf(stderr,
            "usage: solver -x dataset.xml [-s STITCHING|IP] [-l label ..] "
            "[-lw weight ..] [--fixedViews tp,setup[;..]] [--minR 0.3] "
            "[--dryRun]\n");
    return 2;
  }
  const std::string source = args.get("sourcePoints", "STITCHING");
  if (source != "STITCHING" && source != "IP") {
    fprintf(stderr, "error: unknown --sourcePoints %s (STITCHING|IP)\n",
            source.c_str());
    return 2;
  }
  const bool use_ip = source == "IP";
  if (args.get("transformationModel", "TRANSLATION") != "TRANSLATION") {
    fprintf(stderr,
            "error: -tm %s is not supported by this build (TRANSLATION "
            "only)\n",
            args.get("transformationModel").c_str());
    return 2;
  }
  const std::vector<std::string> labels = args.getall("label");
  std::vector<double> label_w;
  for (auto &w : args.getall("labelweights")) label_w.push_back(atof(w.c_str()));
  if (use_ip && labels.empty()) {
    fprintf(stderr, "error: -s IP needs at least one -l label\n");
    return 2;
  }
  if (use_ip && !label_w.empty() && label_w.size() != labels.size()) {
    fprintf(stderr, "error: give one -lw weight per -l label\n");
    return 2;
  }
  bssd::SpimData sd;
  std::string err;
  if (!sd.load(args.get("xml"), &err)) {
    fprintf(stderr, "error: %s\n", err.c_str());
    return 1;
  }
  double minR = args.getd("minR", 0.3);
  std::vector<bssd::StitchEntry> entries;
  if (!use_ip) {
    entries = sd.stitching_results();
    printf("solver: %zu stitching links loaded\n", entries.size());
  }

  /* view index map over (tp, setup) present in registrations */
  std::vector<bssd::ViewId> ids;
  std::map<bssd::ViewId, int> idx;
  for (auto &kv : sd.regs) {
    idx[kv.first] = (int)ids.size();
    ids.push_back(kv.first);
  }
  int n = (int)ids.size();
  if (n == 0) {
    fprintf(stderr, "no registrations\n");
    return 1;
  }
  struct Link {
    int a, b;
    double d[3];
    double w = 1.0; /* [PIN-WEIGHT]: the reference's point matches
      carry the link's correlation as the mpicbg weight
      (ImageCorrelationPointMatchCreator -> PointMatch weight;
      artifact un-vendored, restated as w = r) */
  };
  std::vector<Link> links;
  size_t dropped_hash = 0, dropped_r = 0;
  for (auto &e : entries) {
    if (e.views_a.empty() || e.views_b.empty()) continue;
    auto ia = idx.find(e.views_a[0]);
    auto ib = idx.find(e.views_b[0]);
    if (ia == idx.end() || ib == idx.end()) continue;
    /* hash check against CURRENT registrations (stale links are silently
     * discarded, exactly the reference solver's behaviour) */
    double h = bssd::SpimData::calculate_hash(sd.regs[e.views_a[0]],
                                              sd.regs[e.views_b[0]]);
    if (std::fabs(h - e.hash) > 1e-6 * (1.0 + std::fabs(h))) {
      ++dropped_hash;
      continue;
    }
    if (e.r < minR) {
      ++dropped_r;
      continue;
    }
    Link l;
    l.a = ia->second;
    l.b = ib->second;
    for (int d = 0; d < 3; ++d) l.d[d] = -e.matrix[d * 4 + 3];
    l.w = std::max(0.0, e.r);
    links.push_back(l);
  }
  if (use_ip) {
    const std::string ipn5 = bsip::ipn5_path(args.get("xml"));
    bsn5::Container c(ipn5);
    std::set<std::pair<bssd::ViewId, std::string>> have;
    for (auto &e : sd.interest_points())
      have.insert({{e.timepoint, e.setup}, e.label});
    size_t matches = 0;
    for (size_t li = 0; li < labels.size(); ++li) {
      const std::string &label = labels[li];
      const double lw = label_w.empty() ? 1.0 : label_w[li];
      /* id -> world location per view */
      std::map<bssd::ViewId, std::map<uint64_t, std::array<double, 3>>> world;
      for (auto &v : ids) {
        if (!have.count({v, label})) continue;
        std::vector<uint64_t> pid;
        std::vector<double> loc;
        const std::string group =
            bssd::SpimData::interest_point_group(v.first, v.second, label);
        if (!bsip::read_points(c, group, &pid, &loc)) {
          fprintf(stderr, "error: cannot read %s/%s\n", ipn5.c_str(),
                  group.c_str());
          return 1;
        }
        const auto &m = sd.regs.at(v);
        auto &w = world[v];
        for (size_t i = 0; i < pid.size(); ++i) {
          std::array<double, 3> p;
          for (int r = 0; r < 3; ++r)
            p[r] = m[4 * r] * loc[3 * i] + m[4 * r + 1] * loc[3 * i + 1] +
                   m[4 * r + 2] * loc[3 * i + 2] + m[4 * r + 3];
          w[pid[i]] = p;
        }
      }
      for (auto &va : world) { /* A's list only, partners B > A */
        std::vector<bsip::Corr> list;
        const std::string group = bssd::SpimData::interest_point_group(
            va.first.first, va.first.second, label);
        if (!bsip::read_corrs(c, group, &list)) {
          fprintf(stderr, "error: inconsistent correspondences in %s/%s\n",
                  ipn5.c_str(), group.c_str());
          return 1;
        }
        std::map<bssd::ViewId, std::pair<std::array<double, 3>, size_t>> acc;
        for (auto &k : list) {
          if (k.other_label != label || !(va.first < k.other)) continue;
          auto wb = world.find(k.other);
          if (wb == world.end()) continue;
          auto pa = va.second.find(k.id);
          auto pb = wb->second.find(k.other_id);
          if (pa == va.second.end() || pb == wb->second.end()) continue;
          auto &a = acc[k.other];
          for (int d = 0; d < 3; ++d) a.first[d] += pa->second[d] - pb->second[d];
          ++a.second;
        }
        for (auto &kv : acc) {
          Link l;
          l.a = idx[va.first];
          l.b = idx[kv.first];
          for (int d = 0; d < 3; ++d)
            l.d[d] = kv.second.first[d] / (double)kv.second.second;
          l.w = (double)kv.second.second * lw;
          links.push_back(l);
          matches += kv.second.second;
        }
      }
    }
    printf("solver: %zu interest point links from %zu matches\n",
           links.size(), matches);
  } else {
    printf("solver: %zu usable links (%zu stale-hash, %zu below minR)\n",
           links.size(), dropped_hash, dropped_r);
  }
  if (links.empty()) {
    fprintf(stderr, "nothing to solve\n");
    return 1;
  }

  /* fixed views: default = first view id */
  std::set<int> fixed;
  if (args.has("fixedViews")) {
    std::string spec = args.get("fixedViews");
    std::string cur;
    for (char c : spec + ";") {
      if (c == ';') {
        int tp, su;
        if (sscanf(cur.c_str(), "%d,%d", &tp, &su) == 2) {
          auto it = idx.find({tp, su});
          if (it != idx.end()) fixed.insert(it->second);
        }
        cur.clear();
      } else {
        cur += c;
      }
    }
  }
  if (fixed.empty()) fixed.insert(0);

  /* graph-Laplacian normal equations, solved per axis by dense Gaussian
   * elimination (n = #views is metadata-sized) */
  std::vector<double> t(3 * n, 0.0);
  for (int ax = 0; ax < 3; ++ax) {
    std::vector<double> A((size_t)n * n, 0.0), rhs(n, 0.0);
    for (auto &l : links) {
      A[(size_t)l.a * n + l.a] += l.w;
      A[(size_t)l.b * n + l.b] += l.w;
      A[(size_t)l.a * n + l.b] -= l.w;
      A[(size_t)l.b * n + l.a] -= l.w;
      rhs[l.a] -= l.w * l.d[ax];
      rhs[l.b] += l.w * l.d[ax];
    }
    for (int f : fixed) { /* pin t_f = 0 */
      for (int j = 0; j < n; ++j) A[(size_t)f * n + j] = 0.0;
      A[(size_t)f * n + f] = 1.0;
      rhs[f] = 0.0;
    }
    /* tiny ridge keeps disconnected components solvable */
    for (int i = 0; i < n; ++i) A[(size_t)i * n + i] += 1e-9;
    for (int col = 0; col < n; ++col) { /* partial-pivot elimination */
      int piv = col;
      for (int r = col + 1; r < n; ++r)
        if (std::fabs(A[(size_t)r * n + col]) >
            std::fabs(A[(size_t)piv * n + col]))
          piv = r;
      if (piv != col) {
        for (int j = 0; j < n; ++j)
          std::swap(A[(size_t)col * n + j], A[(size_t)piv * n + j]);
        std::swap(rhs[col], rhs[piv]);
      }
      double p = A[(size_t)col * n + col];
      for (int r = 0; r < n; ++r) {
        if (r == col) continue;
        double f = A[(size_t)r * n + col] / p;
        if (f == 0.0) continue;
        for (int j = col; j < n; ++j)
          A[(size_t)r * n + j] -= f * A[(size_t)col * n + j];
        rhs[r] -= f * rhs[col];
      }
    }
    for (int i = 0; i < n; ++i) t[ax * n + i] = rhs[i] / A[(size_t)i * n + i];
  }

  for (int i = 0; i < n; ++i)
    printf("view (%d,%d): adjustment (%.4f, %.4f, %.4f)\n", ids[i].first,
           ids[i].second, t[0 * n + i], t[1 * n + i], t[2 * n + i]);
  if (args.has("dryRun")) return 0;

  /* prepend the Stitching Transform (outermost) to each registration */
  auto vrs = sd.root->child("ViewRegistrations");
  if (!vrs) {
    fprintf(stderr, "missing ViewRegistrations\n");
    return 1;
  }
  for (auto &vr : vrs->all("ViewRegistration")) {
    int tp = atoi(vr->attrs["timepoint"].c_str());
    int su = atoi(vr->attrs["setup"].c_str());
    auto it = idx.find({tp, su});
    if (it == idx.end()) continue;
    int i = it->second;
    char aff[256];
    snprintf(aff, sizeof aff,
             "1.0 0.0 0.0 %.17g 0.0 1.0 0.0 %.17g 0.0 0.0 1.0 %.17g",
             t[0 * n + i], t[1 * n + i], t[2 * n + i]);
    auto vt = std::make_shared<bsx::Node>();
    vt->tag = "ViewTransform";
    vt->attrs["type"] = "affine";
    vt->add_text("Name",
                 use_ip ? "Interest Point Transform" : "Stitching Transform");
    vt->add_text("affine", aff);
    vr->children.insert(vr->children.begin(), vt);
  }
  if (!sd.save(sd.xml_path)) {
    fprintf(stderr, "cannot write %s\n", sd.xml_path.c_str());
    return 1;
  }
  printf("solver: updated registrations written to %s\n",
         sd.xml_path.c_str());
  return 0;
}
