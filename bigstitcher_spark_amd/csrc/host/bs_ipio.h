/* interestpoints.n5 access shared by match-interestpoints and solver -s IP:
 * reading the point lists detect-interestpoints wrote ([PIN-IPN5],
 * cli_detect.cpp) and reading / writing correspondences.
 *
 * [PIN-IPCORR] restates mvrecon's
 * InterestPointsN5.saveCorrespondingInterestPoints (artifact un-vendored):
 * under {tpId_T_viewSetupId_S}/{label}/correspondences the attributes
 * correspondences "1.0.0" and idMap {"tp,setup,label": k}, and the dataset
 * `data`, uint64 [3, N], block [3, 300000], zstd, whose rows are (own
 * detection id, corresponding detection id, idMap value of the other
 * view/label). No `data` dataset = no correspondences. */
#ifndef BS_IPIO_H
#define BS_IPIO_H

#include <cstdint>
#include <cstdio>
#include <filesystem>
#include <map>
#include <string>
#include <vector>

#include "bs_n5.h"
#include "bs_spimdata.h"

namespace bsip {

const int IP_BLOCK = 300000; /* InterestPointsN5.defaultBlockSize */

inline std::string ipn5_path(const std::string &xml) {
  namespace fs = std::filesystem;
  fs::path xmlp(xml);
  return (xmlp.has_parent_path() ? xmlp.parent_path() : fs::path("."))
      .append("interestpoints.n5")
      .string();
}

/* [rows, N] dataset in [rows, IP_BLOCK] blocks -> N * rows elements */
template <typename T>
bool read_2d(const bsn5::Container &c, const std::string &name,
             const std::string &dtype, int rows, std::vector<T> *out) {
  bsn5::DatasetAttrs a;
  if (!c.get_dataset_attrs(name, &a) || a.dtype != dtype ||
      a.dims.size() != 2 || a.dims[0] != rows || a.block.size() != 2 ||
      a.block[0] != rows || a.block[1] < 1 || a.dims[1] < 0 ||
      bsn5::dtype_size(dtype) != sizeof(T))
    return false;
  const size_t n = (size_t)a.dims[1], bn = (size_t)a.block[1];
  out->assign(n * rows, T());
  std::vector<T> buf(bn * rows);
  for (size_t g = 0; g * bn < n; ++g) {
    const size_t cn = std::min(bn, n - g * bn);
    std::vector<int> clipped;
    if (!c.read_block(name, a, {0, (long long)g}, buf.data(), &clipped) ||
        clipped.size() != 2 || clipped[0] != rows || (size_t)clipped[1] != cn)
      return false;
    std::copy(buf.begin(), buf.begin() + cn * rows,
              out->begin() + g * bn * rows);
  }
  return true;
}

template <typename T>
bool write_2d(bsn5::Container &c, const std::string &name,
              const std::string &dtype, int rows, size_t n, const T *data) {
  bsn5::DatasetAttrs a;
  a.dims = {rows, (long long)n};
  a.block = {rows, IP_BLOCK};
  a.dtype = dtype;
  a.compression = "zstd";
  if (!c.create_dataset(name, a)) return false;
  for (size_t g = 0; g * IP_BLOCK < n; ++g) {
    const size_t cn = std::min((size_t)IP_BLOCK, n - g * IP_BLOCK);
    if (!c.write_block(name, a, {0, (long long)g},
                       data + g * IP_BLOCK * rows, {rows, (int)cn}))
      return false;
  }
  return true;
}

/* ids and full-resolution view-local locations of one view/label */
inline bool read_points(const bsn5::Container &c, const std::string &group,
                        std::vector<uint64_t> *ids, std::vector<double> *loc) {
  const std::string g = group + "/interestpoints";
  return read_2d<uint64_t>(c, g + "/id", "uint64", 1, ids) &&
         read_2d<double>(c, g + "/loc", "float64", 3, loc) &&
         loc->size() == 3 * ids->size();
}

struct Corr {
  uint64_t id = 0, other_id = 0;
  bssd::ViewId other{0, 0};
  std::string other_label;
};

inline std::string corr_key(const bssd::ViewId &v, const std::string &label) {
  return std::to_string(v.first) + "," + std::to_string(v.second) + "," +
         label;
}

/* false only when the stored data is inconsistent; a group without `data`
 * gives an empty list */
inline bool read_corrs(const bsn5::Container &c, const std::string &group,
                       std::vector<Corr> *out) {
  out->clear();
  const std::string g = group + "/correspondences";
  auto idmap = c.get_attr(g, "idMap");
  bsn5::DatasetAttrs a;
  if (!c.get_dataset_attrs(g + "/data", &a)) return true;
  std::vector<uint64_t> rows;
  if (!read_2d<uint64_t>(c, g + "/data", "uint64", 3, &rows)) return false;
  std::map<uint64_t, std::pair<bssd::ViewId, std::string>> rev;
  if (idmap && idmap->type == bsj::Value::OBJ)
    for (auto &kv : idmap->obj) {
      int tp = 0, su = 0, used = 0;
      if (sscanf(kv.first.c_str(), "%d,%d,%n", &tp, &su, &used) < 2 || !used)
        return false;
      rev[(uint64_t)kv.second->inum] = {{tp, su}, kv.first.substr(used)};
    }
  for (size_t i = 0; i + 2 < rows.size(); i += 3) {
    auto it = rev.find(rows[i + 2]);
    if (it == rev.end()) return false;
    Corr k;
    k.id = rows[i];
    k.other_id = rows[i + 1];
    k.other = it->second.first;
    k.other_label = it->second.second;
    out->push_back(k);
  }
  return true;
}

inline bool write_corrs(bsn5::Container &c, const std::string &group,
                        const std::vector<Corr> &list) {
  namespace fs = std::filesystem;
  const std::string g = group + "/correspondences";
  std::error_code ec;
  fs::remove_all(fs::path(c.root()) / g / "data", ec);
  std::map<std::string, uint64_t> idmap; /* keys numbered in first-use order */
  std::vector<uint64_t> rows;
  rows.reserve(list.size() * 3);
  for (auto &k : list) {
    const std::string key = corr_key(k.other, k.other_label);
    auto it = idmap.find(key);
    if (it == idmap.end()) it = idmap.emplace(key, idmap.size()).first;
    rows.push_back(k.id);
    rows.push_back(k.other_id);
    rows.push_back(it->second);
  }
  auto jm = bsj::Value::mkobj();
  for (auto &kv : idmap)
    jm->obj[kv.first] = bsj::Value::mkint((long long)kv.second);
  if (!c.set_attr(g, "correspondences", bsj::Value::mkstr("1.0.0")) ||
      !c.set_attr(g, "idMap", jm))
    return false;
  if (list.empty()) return true;
  return write_2d<uint64_t>(c, g + "/data", "uint64", 3, list.size(),
                            rows.data());
}

}  // namespace bsip

#endif
