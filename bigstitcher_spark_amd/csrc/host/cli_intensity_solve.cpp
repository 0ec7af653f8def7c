/* `solve-intensities` — drop-in for the reference's IntensitySolver CLI
 * (flag surface: IntensitySolver.java:29-48). Reads every view pair's
 * matches from the [PIN-INTMATCH-IO] container that `match-intensities`
 * wrote (bs_intio.h; reference :100-111), runs bs_intensity_solve (the
 * IntensityCorrection.solve replacement, :116; [PIN-INT-SOLVE],
 * csrc/bs_intensity_solve.h) and writes one float64 dataset of dims
 * {gx, gy, gz, 2} per view at
 *   {--intensityN5Group}/setup{s}/timepoint{t}/{--intensityN5Dataset}
 * which is where `affine-fusion --intensityN5Path` looks for it.
 * Host only: needs no GPU and does not link the HIP library. Beyond the
 * reference's flags: --lambdaIdentity (0.01) and --lambdaSmooth (0.1). */
#include <cstdio>
#include <map>

#include "../bs_intensity_solve.h"
#include "bs_cli_util.h"
#include "bs_intio.h"
#include "bs_n5.h"
#include "bs_spimdata.h"

static std::string strip_file_uri(const std::string &s) {
  return s.rfind("file:", 0) == 0 ? s.substr(5) : s;
}

int main(int argc, char **argv) {
  bscli::Args args;
  std::map<std::string, std::string> alias = {
      {"-x", "--xml"},
      {"-o", "--intensityN5Path"},
      {"-s", "--intensityN5Storage"},
      {"-vi", "--vi"}};
  const char *usage =
      "usage: solve-intensities -x dataset.xml --matchesPath matches.n5 "
      "-o coefficients.n5 [--numCoefficients 8,8,8] [--maxIterations 1000] "
      "[--intensityN5Group g] [--intensityN5Dataset intensity] "
      "[--lambdaIdentity 0.01] [--lambdaSmooth 0.1] [-vi 'tp,setup' ... | "
      "--angleId/--tileId/--channelId/--illuminationId/--timepointId "
      "'0,1,..']\n";
  if (!args.parse(argc, argv, alias, {"localSparkBindAddress"})) {
    fputs(usage, stderr);
    return 2;
  }
  for (const char *f : {"xml", "matchesPath", "intensityN5Path"})
    if (!args.has(f)) {
      fprintf(stderr, "error: missing required option --%s\n", f);
      fputs(usage, stderr);
      return 2;
    }
  const std::string outp = strip_file_uri(args.get("intensityN5Path"));
  std::string storage = args.get("intensityN5Storage");
  if (storage.empty()) {
    auto ends = [&](const char *e) {
      const std::string s(e);
      return outp.size() >= s.size() &&
             outp.compare(outp.size() - s.size(), s.size(), s) == 0;
    };
    storage = ends(".h5") || ends(".hdf5") ? "HDF5"
              : ends(".zarr")              ? "ZARR"
                                           : "N5";
  }
  if (storage != "N5") {
    fprintf(stderr, "error: coefficient storage %s is not built (N5 only)\n",
            storage.c_str());
    return 2;
  }
  auto nc = bscli::parse_ints(args.get("numCoefficients", "8,8,8"));
  if (nc.size() != 3 || nc[0] < 1 || nc[1] < 1 || nc[2] < 1) {
    fprintf(stderr, "error: --numCoefficients needs three counts >= 1\n");
    return 2;
  }
  const int32_t cg[3] = {(int32_t)nc[0], (int32_t)nc[1], (int32_t)nc[2]};
  bs_intensity_solve_params prm{};
  prm.lambda_identity = args.getd("lambdaIdentity", 0.01);
  prm.lambda_smooth = args.getd("lambdaSmooth", 0.1);
  prm.max_iterations = (int32_t)args.getl("maxIterations", 1000);
  if (prm.max_iterations < 1 || prm.lambda_identity < 0 ||
      prm.lambda_smooth < 0) {
    fprintf(stderr, "error: need --maxIterations >= 1 and lambdas >= 0\n");
    return 2;
  }

  bssd::SpimData sd;
  std::string err;
  if (!sd.load(args.get("xml"), &err)) {
    fprintf(stderr, "error: %s\n", err.c_str());
    return 1;
  }
  std::vector<bssd::ViewId> views;
  if (!bssd::select_views(sd, args.getall("vi"), args.get("angleId"),
                          args.get("tileId"), args.get("illuminationId"),
                          args.get("channelId"), args.get("timepointId"),
                          &views, &err)) {
    fprintf(stderr, "error: %s\n", err.c_str());
    return 1;
  }
  if (views.empty()) {
    fprintf(stderr, "error: no views selected\n");
    return 1;
  }
  bsn5::Container in(strip_file_uri(args.get("matchesPath")));
  int32_t stored[3];
  if (!bsint_io::read_coefficients_size(in, stored)) {
    fprintf(stderr, "error: %s holds no coefficientsSize attribute\n",
            in.root().c_str());
    return 1;
  }
  if (stored[0] != cg[0] || stored[1] != cg[1] || stored[2] != cg[2])
    fprintf(stderr, "numCoefficients stored with matches is different from "
                    "specified numCoefficients argument!\n");

  std::vector<int32_t> pair_views;
  std::vector<size_t> offsets = {0};
  std::vector<bs_intensity_match> all;
  for (size_t i = 0; i < views.size(); ++i)
    for (size_t j = i + 1; j < views.size(); ++j) {
      std::vector<bs_intensity_match> m;
      if (!bsint_io::read_pair(in, views[i], views[j], &m) || m.empty())
        continue;
      pair_views.push_back((int32_t)i);
      pair_views.push_back((int32_t)j);
      all.insert(all.end(), m.begin(), m.end());
      offsets.push_back(all.size());
    }
  const size_t npairs = offsets.size() - 1;
  printf("Connected pairs: %zu (%zu buckets)\nRunning solve...\n", npairs,
         all.size());
  const size_t ncell = (size_t)cg[0] * cg[1] * cg[2];
  std::vector<double> coeff(views.size() * 2 * ncell);
  int32_t iters = 0;
  double relres = 0;
  const int rc = bs_intensity_solve(
      (int32_t)views.size(), cg, pair_views.data(), offsets.data(), npairs,
      all.data(), &prm, coeff.data(), &iters, &relres);
  if (rc != BS_OK) {
    fprintf(stderr, "error: solve failed (rc=%d): a match refers to a cell "
                    "outside --numCoefficients\n", rc);
    return 1;
  }
  printf("solve: %d iterations, relative residual %.3e\n", iters, relres);

  printf("Writing coefficients to: %s\n", outp.c_str());
  bsn5::Container out(outp);
  if (!out.create()) {
    fprintf(stderr, "error: cannot create %s\n", outp.c_str());
    return 1;
  }
  const std::string group = args.get("intensityN5Group", "");
  const std::string dsname = args.get("intensityN5Dataset", "intensity");
  for (size_t v = 0; v < views.size(); ++v) {
    const std::string name =
        (group.empty() ? std::string() : group + "/") + "setup" +
        std::to_string(views[v].second) + "/timepoint" +
        std::to_string(views[v].first) + "/" + dsname;
    bsn5::DatasetAttrs at;
    at.dims = {cg[0], cg[1], cg[2], 2};
    at.block = {cg[0], cg[1], cg[2], 2};
    at.dtype = "float64";
    at.compression = "raw";
    if (!out.create_dataset(name, at) ||
        !out.write_block(name, at, {0, 0, 0, 0}, &coeff[v * 2 * ncell],
                         {cg[0], cg[1], cg[2], 2})) {
      fprintf(stderr, "error: cannot write %s\n", name.c_str());
      return 1;
    }
  }
  printf("Done.\n");
  return 0;
}
