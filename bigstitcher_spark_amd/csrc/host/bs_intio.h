/* Intensity-match container shared by `match-intensities` (writer) and
 * `solve-intensities` (reader). [PIN-INTMATCH-IO] is this project's own
 * layout (mvrecon's ViewPairCoefficientMatchesIO is un-vendored; a stock
 * Java tool may not read it): an N5 group holding
 *   attribute "coefficientsSize": [gx, gy, gz]
 *   one uint64 dataset per view pair,
 *     matches/tp{t1}_setup{s1}__tp{t2}_setup{s2}, dims {11, nbuckets},
 *   one column per accepted bucket: cell_a, cell_b, n_cand, n_inl, best_it,
 *   n_inl_first, sp, sq, spp, sqq, spq (bs_intensity_match without a, b,
 *   which follow from the moments). A pair without accepted buckets has a
 *   dataset of dims {11, 0} and no block. */
#ifndef BS_INTIO_H
#define BS_INTIO_H

#include <string>
#include <vector>

#include "../../../include/bigstitch.h"
#include "bs_n5.h"
#include "bs_spimdata.h"

namespace bsint_io {

const int FIELDS = 11;

inline std::string pair_dataset(const bssd::ViewId &a, const bssd::ViewId &b) {
  return "matches/tp" + std::to_string(a.first) + "_setup" +
         std::to_string(a.second) + "__tp" + std::to_string(b.first) +
         "_setup" + std::to_string(b.second);
}

inline bool write_coefficients_size(bsn5::Container &c, const int32_t cg[3]) {
  return c.set_attr("", "coefficientsSize",
                    bsj::Value::mkints(std::vector<int>{cg[0], cg[1], cg[2]}));
}

inline bool read_coefficients_size(const bsn5::Container &c, int32_t cg[3]) {
  auto v = c.get_attr("", "coefficientsSize");
  if (!v || v->type != bsj::Value::ARR || v->arr.size() != 3) return false;
  for (int d = 0; d < 3; ++d) cg[d] = (int32_t)v->arr[d]->num;
  return true;
}

inline bool write_pair(bsn5::Container &c, const bssd::ViewId &a,
                       const bssd::ViewId &b,
                       const std::vector<bs_intensity_match> &m) {
  const std::string name = pair_dataset(a, b);
  bsn5::DatasetAttrs at;
  at.dims = {FIELDS, (long long)m.size()};
  at.block = {FIELDS, (int)std::max<size_t>(m.size(), 1)};
  at.dtype = "uint64";
  at.compression = "raw";
  if (!c.create_dataset(name, at)) return false;
  if (m.empty()) return true;
  std::vector<uint64_t> buf(m.size() * FIELDS);
  for (size_t i = 0; i < m.size(); ++i) {
    const uint64_t f[FIELDS] = {m[i].cell_a, m[i].cell_b, m[i].n_cand,
                                m[i].n_inl,  m[i].best_it, m[i].n_inl_first,
                                m[i].sp,     m[i].sq,      m[i].spp,
                                m[i].sqq,    m[i].spq};
    for (int k = 0; k < FIELDS; ++k) buf[i * FIELDS + k] = f[k];
  }
  return c.write_block(name, at, {0, 0}, buf.data(), {FIELDS, (int)m.size()});
}

/* false when the pair has no dataset; a, b of each match are left zero */
inline bool read_pair(const bsn5::Container &c, const bssd::ViewId &a,
                      const bssd::ViewId &b,
                      std::vector<bs_intensity_match> *m) {
  const std::string name = pair_dataset(a, b);
  bsn5::DatasetAttrs at;
  m->clear();
  if (!c.get_dataset_attrs(name, &at) || at.dims.size() != 2 ||
      at.dims[0] != FIELDS || at.dtype != "uint64" || at.block.size() != 2 ||
      at.block[0] != FIELDS || at.block[1] < 1)
    return false;
  const long long n = at.dims[1];
  std::vector<uint64_t> blk((size_t)FIELDS * at.block[1]);
  for (long long g = 0; g * at.block[1] < n; ++g) {
    std::vector<int> cd;
    if (!c.read_block(name, at, {0, g}, blk.data(), &cd) || cd.size() != 2 ||
        cd[0] != FIELDS)
      return false;
    for (int i = 0; i < cd[1]; ++i) {
      const uint64_t *f = &blk[(size_t)i * FIELDS];
      bs_intensity_match r{};
      r.cell_a = f[0]; r.cell_b = f[1]; r.n_cand = f[2]; r.n_inl = f[3];
      r.best_it = f[4]; r.n_inl_first = f[5]; r.sp = f[6]; r.sq = f[7];
      r.spp = f[8]; r.sqq = f[9]; r.spq = f[10];
      m->push_back(r);
    }
  }
  return (long long)m->size() == n;
}

}  // namespace bsint_io

#endif
