/* `detect-interestpoints` — drop-in for the reference's
 * SparkInterestPointDetection CLI (flag surface:
 * SparkInterestPointDetection.java:116-170; pipeline: :176-971). The host
 * opens each selected view at the pyramid level the reference would pick
 * (:1033-1045), runs libbigstitch's bs_detect_dog (the
 * DoGImgLib2.computeDoG replacement, :552-568) with the remaining
 * downsampling as residual box-mean factors, maps the points back to full
 * resolution ([PIN-MIP]), optionally keeps the --maxSpots brightest
 * (filterPoints, :973-995), and writes interestpoints.n5 beside the XML
 * plus the <ViewInterestPoints> entries (:894-910).
 *
 * Whole views are processed at once (the reference tiles them into
 * --blockSize jobs only to fit Spark executors; the result of DoG + extrema
 * does not depend on that tiling). Not supported, refused with exit 2:
 * --overlappingOnly, --onlyCompareOverlapTiles, --maxSpotsPerOverlap,
 * --medianFilter, --prefetch, --keepTemporaryN5.
 *
 * [PIN-IPN5] restates mvrecon's InterestPointsN5 layout (artifact
 * un-vendored): group tpId_{t}_viewSetupId_{s}/{label}/interestpoints
 * {pointcloud "1.0.0", type "list", list version "1.0.0"} with datasets
 * id (uint64 [1,N]) and loc (float64 [3,N]), block [*,300000], zstd; the
 * sibling group .../correspondences {correspondences "1.0.0", idMap {}};
 * intensities (float32 [1,N]) with --storeIntensities. */
#include <cinttypes>
#include <cstdio>
#include <filesystem>
#include <numeric>

#include "../../../include/bigstitch.h"
#include "bs_cli_util.h"
#include "bs_imgio.h"
#include "bs_mip.h"
#include "bs_n5.h"
#include "bs_spimdata.h"

namespace {

const int IP_BLOCK = 300000; /* InterestPointsN5.defaultBlockSize */

/* Java's Double.toString for the params attribute ([PIN-IPXML], reference
 * :905-906 concatenates Double objects): shortest round-trip decimal with
 * at least one fraction digit; computerized scientific notation outside
 * [1e-3, 1e7). */
std::string java_double(double v) {
  char buf[64];
  int prec = 1;
  for (; prec <= 17; ++prec) {
    snprintf(buf, sizeof buf, "%.*e", prec - 1, v);
    if (strtod(buf, nullptr) == v) break;
  }
  /* buf = d.ddddE[+-]xx */
  std::string s(buf);
  size_t epos = s.find('e');
  std::string mant = s.substr(0, epos);
  int ex = atoi(s.c_str() + epos + 1);
  bool neg = !mant.empty() && mant[0] == '-';
  if (neg) mant = mant.substr(1);
  std::string digits;
  for (char c : mant)
    if (c != '.') digits += c;
  std::string out;
  double a = std::fabs(v);
  if (v == 0) {
    out = "0.0";
  } else if (a >= 1e-3 && a < 1e7) {
    if (ex >= 0) {
      while ((int)digits.size() < ex + 1) digits += '0';
      out = digits.substr(0, ex + 1) + ".";
      std::string frac = digits.substr(ex + 1);
      out += frac.empty() ? "0" : frac;
    } else {
      out = "0." + std::string(-ex - 1, '0') + digits;
    }
  } else {
    out = digits.substr(0, 1) + "." +
          (digits.size() > 1 ? digits.substr(1) : "0") + "E" +
          std::to_string(ex);
  }
  return neg ? "-" + out : out;
}

bool is_pow2(long long v) { return v >= 1 && (v & (v - 1)) == 0; }

/* [rows, N] dataset written in [rows, IP_BLOCK] blocks; N = 0 writes the
 * attributes only */
bool write_2d(bsn5::Container &c, const std::string &name,
              const std::string &dtype, int rows, size_t n,
              const void *data) {
  bsn5::DatasetAttrs a;
  a.dims = {rows, (long long)n};
  a.block = {rows, IP_BLOCK};
  a.dtype = dtype;
  a.compression = "zstd";
  if (!c.create_dataset(name, a)) return false;
  const size_t esz = bsn5::dtype_size(dtype);
  for (size_t g = 0; g * IP_BLOCK < n; ++g) {
    const size_t cn = std::min((size_t)IP_BLOCK, n - g * IP_BLOCK);
    if (!c.write_block(name, a, {0, (long long)g},
                       (const char *)data + g * IP_BLOCK * rows * esz,
                       {rows, (int)cn}))
      return false;
  }
  return true;
}

}  // namespace

int main(int argc, char **argv) {
  bscli::Args args;
  std::map<std::string, std::string> alias = {
      {"-x", "--xml"},           {"-l", "--label"},
      {"-s", "--sigma"},         {"-t", "--threshold"},
      {"-i0", "--minIntensity"}, {"-i1", "--maxIntensity"},
      {"-dsxy", "--downsampleXY"}, {"-dsz", "--downsampleZ"},
      {"-vi", "--vi"}};
  const char *usage =
      "usage: detect-interestpoints -x dataset.xml -l label -s sigma "
      "-t threshold -i0 minIntensity -i1 maxIntensity [--type MIN|MAX|BOTH] "
      "[--localization NONE|QUADRATIC] [-dsxy 2] [-dsz 1] [--maxSpots N] "
      "[--storeIntensities] [-vi 'tp,setup' ... | --angleId/--tileId/"
      "--channelId/--illuminationId/--timepointId '0,1,..'] [--device N] "
      "[--dryRun]\n";
  if (!args.parse(argc, argv, alias,
                  {"storeIntensities", "dryRun", "overlappingOnly",
                   "onlyCompareOverlapTiles", "maxSpotsPerOverlap",
                   "prefetch", "keepTemporaryN5", "localSparkBindAddress"})) {
    fputs(usage, stderr);
    return 2;
  }
  /* refused before anything else happens (no XML read, no GPU call) */
  for (const char *f : {"overlappingOnly", "onlyCompareOverlapTiles",
                        "maxSpotsPerOverlap", "medianFilter", "prefetch",
                        "keepTemporaryN5"})
    if (args.has(f)) {
      fprintf(stderr, "error: --%s is not supported by this build\n", f);
      return 2;
    }
  for (const char *f : {"xml", "label", "sigma", "threshold", "minIntensity",
                        "maxIntensity"})
    if (!args.has(f)) {
      fprintf(stderr, "error: missing required option --%s\n", f);
      fputs(usage, stderr);
      return 2;
    }
  for (const char *f : {"s3Region", "localSparkBindAddress", "blockSize"})
    if (args.has(f))
      fprintf(stderr, "note: --%s accepted for compatibility (no-op in "
                      "this build)\n", f);
  const std::string label = args.get("label");
  const std::string type = args.get("type", "MAX");
  const std::string locz = args.get("localization", "QUADRATIC");
  if (type != "MIN" && type != "MAX" && type != "BOTH") {
    fprintf(stderr, "error: unsupported --type %s (MIN|MAX|BOTH)\n",
            type.c_str());
    return 2;
  }
  if (locz != "NONE" && locz != "QUADRATIC") {
    fprintf(stderr,
            "error: unsupported --localization %s (NONE|QUADRATIC)\n",
            locz.c_str());
    return 2;
  }
  const long long dsxy = args.getl("downsampleXY", 2),
                  dsz = args.getl("downsampleZ", 1);
  if (!is_pow2(dsxy) || !is_pow2(dsz) || dsxy > 128 || dsz > 128) {
    fprintf(stderr, "error: -dsxy/-dsz must be powers of two in 1..128\n");
    return 2;
  }
  const long maxSpots = args.getl("maxSpots", -1);
  const bool storeIntensities = args.has("storeIntensities");
  const bool dryRun = args.has("dryRun");
  const bool findMin = type == "MIN" || type == "BOTH";
  const bool findMax = type == "MAX" || type == "BOTH";

  bs_dog_params prm{};
  prm.sigma = args.getd("sigma", 0);
  prm.threshold = args.getd("threshold", 0);
  prm.min_intensity = args.getd("minIntensity", 0);
  prm.max_intensity = args.getd("maxIntensity", 0);
  prm.find_min = findMin;
  prm.find_max = findMax;
  prm.localization = locz == "QUADRATIC" ? 1 : 0;
  if (!(prm.sigma > 0.5) || prm.max_intensity == prm.min_intensity) {
    fprintf(stderr, "error: need --sigma > 0.5 and --minIntensity != "
                    "--maxIntensity\n");
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
  printf("detect-interestpoints: %zu views, label '%s', sigma %s threshold "
         "%s, %s %s, container %s\n",
         selected.size(), label.c_str(), java_double(prm.sigma).c_str(),
         java_double(prm.threshold).c_str(), type.c_str(), locz.c_str(),
         sd.n5_path.c_str());

  bsimg::Input input(sd);
  bs_ctx *ctx = nullptr;
  if (bs_ctx_create(&ctx, (int)args.getl("device", 0)) != BS_OK) {
    fprintf(stderr, "error: %s\n", bs_last_error(nullptr));
    return 1;
  }

  struct ViewPoints {
    bssd::ViewId id;
    std::vector<double> loc; /* 3 per point, full-resolution view px */
    std::vector<float> intensity;
  };
  std::vector<ViewPoints> results;
  const long long want[3] = {dsxy, dsxy, dsz};
  for (auto &vid : selected) {
    const int tp = vid.first, setup = vid.second;
    /* level pick, reference :1033-1045: the LAST level whose integer
     * factors are all <= the requested ones and powers of two */
    auto levels = input.read_levels(setup, tp);
    long long f[3] = {1, 1, 1};
    int level = 0;
    for (auto &lv : levels)
      if (lv.f[0] <= want[0] && lv.f[1] <= want[1] && lv.f[2] <= want[2] &&
          is_pow2(lv.f[0]) && is_pow2(lv.f[1]) && is_pow2(lv.f[2]) &&
          lv.f[0] <= 128 && lv.f[1] <= 128 && lv.f[2] <= 128) {
        level = lv.level;
        for (int d = 0; d < 3; ++d) f[d] = lv.f[d];
      }
    for (int d = 0; d < 3; ++d) prm.ds[d] = (int32_t)(want[d] / f[d]);
    std::vector<uint16_t> vox;
    std::vector<long long> dims;
    if (!input.read_volume_u16(setup, tp, level, &vox, &dims)) {
      fprintf(stderr, "cannot read view tp=%d setup=%d level %d from %s\n",
              tp, setup, level, sd.n5_path.c_str());
      return 1;
    }
    const int64_t d3[3] = {dims[0], dims[1], dims[2]};
    if (bs_view_upload(ctx, setup, vox.data(), d3) != BS_OK) {
      fprintf(stderr, "upload failed: %s\n", bs_last_error(ctx));
      return 1;
    }
    size_t n = 0;
    int rc = bs_detect_dog(ctx, setup, &prm, nullptr, 0, &n);
    std::vector<bs_interest_point> pts(n);
    if (rc == BS_OK && n)
      rc = bs_detect_dog(ctx, setup, &prm, pts.data(), pts.size(), &n);
    if (rc != BS_OK || n != pts.size()) {
      fprintf(stderr, "detection failed for view (%d,%d): rc=%d %s\n", tp,
              setup, rc, bs_last_error(ctx));
      return 1;
    }
    (void)bs_view_release(ctx, setup);
    printf("view (%d,%d): level %d ds %lld,%lld,%lld residual %d,%d,%d: "
           "%zu interest points\n",
           tp, setup, level, f[0], f[1], f[2], prm.ds[0], prm.ds[1],
           prm.ds[2], n);
    /* --maxSpots: the N largest intensities, renumbered (:973-995) */
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    if (maxSpots > 0 && n > (size_t)maxSpots) {
      std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        return pts[a].intensity > pts[b].intensity;
      });
      order.resize((size_t)maxSpots);
      printf("view (%d,%d): --maxSpots kept the %ld brightest\n", tp, setup,
             maxSpots);
    }
    ViewPoints vp;
    vp.id = vid;
    for (size_t i : order) {
      for (int d = 0; d < 3; ++d) /* [PIN-MIP] level px -> full-res px */
        vp.loc.push_back((double)f[d] * pts[i].loc[d] +
                         ((double)f[d] - 1.0) * 0.5);
      vp.intensity.push_back(pts[i].intensity);
    }
    results.push_back(std::move(vp));
  }
  bs_ctx_destroy(ctx);

  if (dryRun) {
    printf("--dryRun: nothing written\n");
    return 0;
  }

  /* [PIN-IPN5] interestpoints.n5 beside the XML */
  namespace fs = std::filesystem;
  fs::path xmlp(args.get("xml"));
  const std::string ipn5 =
      (xmlp.has_parent_path() ? xmlp.parent_path() : fs::path("."))
          .append("interestpoints.n5")
          .string();
  bsn5::Container c(ipn5);
  if (!c.create()) {
    fprintf(stderr, "error: cannot create %s\n", ipn5.c_str());
    return 1;
  }
  /* params string of reference :905-906 */
  const std::string params =
      "DOG (Spark) s=" + java_double(prm.sigma) +
      " t=" + java_double(prm.threshold) + " overlappingOnly=false" +
      " min=" + (findMin ? "true" : "false") +
      " max=" + (findMax ? "true" : "false") +
      " downsampleXY=" + std::to_string(dsxy) +
      " downsampleZ=" + std::to_string(dsz) +
      " minIntensity=" + java_double(prm.min_intensity) +
      " maxIntensity=" + java_double(prm.max_intensity);
  for (auto &vp : results) {
    const std::string group = bssd::SpimData::interest_point_group(
        vp.id.first, vp.id.second, label);
    std::error_code ec;
    fs::remove_all(fs::path(ipn5) / group, ec); /* replace, never merge */
    const std::string ipg = group + "/interestpoints";
    const size_t n = vp.intensity.size();
    std::vector<uint64_t> ids(n);
    std::iota(ids.begin(), ids.end(), (uint64_t)0);
    bool ok = c.set_attr(ipg, "pointcloud", bsj::Value::mkstr("1.0.0")) &&
              c.set_attr(ipg, "type", bsj::Value::mkstr("list")) &&
              c.set_attr(ipg, "list version", bsj::Value::mkstr("1.0.0")) &&
              write_2d(c, ipg + "/id", "uint64", 1, n, ids.data()) &&
              write_2d(c, ipg + "/loc", "float64", 3, n, vp.loc.data());
    if (ok && storeIntensities)
      ok = write_2d(c, ipg + "/intensities", "float32", 1, n,
                    vp.intensity.data());
    const std::string cg = group + "/correspondences";
    ok = ok &&
         c.set_attr(cg, "correspondences", bsj::Value::mkstr("1.0.0")) &&
         c.set_attr(cg, "idMap", bsj::Value::mkobj());
    if (!ok) {
      fprintf(stderr, "error: cannot write %s/%s\n", ipn5.c_str(),
              group.c_str());
      return 1;
    }
    bssd::InterestPointEntry e;
    e.timepoint = vp.id.first;
    e.setup = vp.id.second;
    e.label = label;
    e.params = params;
    e.path = group;
    sd.set_interest_points(e); /* views with zero detections too (:896-900) */
  }
  if (!sd.save(args.get("xml"))) {
    fprintf(stderr, "error: cannot write %s\n", args.get("xml").c_str());
    return 1;
  }
  printf("saved %zu views to %s and %s\n", results.size(), ipn5.c_str(),
         args.get("xml").c_str());
  return 0;
}
