// cms_covis_core.h -- the numeric core of the covisibility bookkeeping: KeyFrame::UpdateConnections (src/KeyFrame.cpp:315-404),
// LocalMapping::KeyFrameCulling (src/LocalMapping.cpp:561-619), the votes of Tracking::UpdateLocalKeyFrames (src/Tracking.cpp:881-928) and
// Tracking::UpdateLocalPoints (:855-878), on plain arrays.  ONE source for the host build (libcubemapslam_host.so: hm_covis_*, the definition of
// record) and for the gfx950 kernels (cms_covis_kernels.hip).  It compiles under g++ as it stands.
//
// The observation index is built over a list of MEMBER rows: member m has n[m] features, each with a map-point id (mp, < 0: none or bad) and
// an octave.  An observation is (id, member position, feature, octave) for every feature with mp >= 0; Observations(id) is the number of members
// that hold the id (MapPoint::nObs of this monocular system).  Ids are arbitrary ints in [0, 2^30): nothing is indexed by id.  An id may appear
// once per row (MapPoint::AddObservation's invariant); a row that repeats one makes the build fail and the previous index stays.
//
// Everything is integer work: counts, lists and flags.  The one place the reference leaves open is the order of equal weights in
// mvpOrderedConnectedKeyFrames (it sorts pair<int, KeyFrame*>, so the pointer decides): here the EARLIER member position goes first
// (cms_covis_before), and a maximum is the earliest member that attains it (map<KeyFrame*, int> iteration with a strict >).
#ifndef CMS_COVIS_CORE_H
#define CMS_COVIS_CORE_H
#include <stdint.h>
#include "cms_detmath.h"      // CMS_HD

#define CMS_COVIS_MAX_MEMBERS 16384      // the database's bound (CMS_KFDB_MAX_ENTRIES)
#define CMS_COVIS_MAX_ID 0x3FFFFFFF      // ids are mnId & 0x3FFFFFFF

// scaleLeveli <= scaleLevel + 1 (LocalMapping.cpp:600)
CMS_HD bool cms_covis_octave_ok(int octave_i, int octave) { return octave_i <= octave + 1; }
// nRedundantObservations > 0.9*nMPs (LocalMapping.cpp:616): an int against a double product
CMS_HD bool cms_covis_redundant(int n_redundant, int n_mps) { return (double)n_redundant > 0.9 * (double)n_mps; }
// nObs <= 2 after an erased observation: the point is discarded (MapPoint.cpp:129)
CMS_HD bool cms_covis_point_dies(int n_obs_left) { return n_obs_left <= 2; }
// the place of member a in front of member b in mvpOrderedConnectedKeyFrames: descending weight, ties to the earlier member position
CMS_HD bool cms_covis_before(int w_a, int pos_a, int w_b, int pos_b) { return w_a > w_b || (w_a == w_b && pos_a < pos_b); }
// one int that orders (weight, earlier position first) for a maximum: weights are at most 16383 features, positions below 16384
CMS_HD int cms_covis_max_key(int w, int pos) { return (w << 14) | (CMS_COVIS_MAX_MEMBERS - 1 - pos); }
CMS_HD int cms_covis_max_key_pos(int key) { return CMS_COVIS_MAX_MEMBERS - 1 - (key & (CMS_COVIS_MAX_MEMBERS - 1)); }
// where an id starts to probe a table of 2^bits entries (the kernels' open-addressing table; any spread would do: the table's order is unspecified)
CMS_HD uint32_t cms_covis_hash(int id, int bits) { return ((uint32_t)id * 2654435761u) >> (32 - bits); }

// ---------------------------------------------------------------------------------------------------------------------------------------------
// host only from here: the index of record
#include <algorithm>
#include <vector>

struct CmsCovisHost {
  struct Obs { int id, member, feat, octave; };
  int n_members = 0;
  std::vector<std::vector<int>> mp, oct;      // the snapshot of the members' rows
  std::vector<Obs> obs;                       // sorted by (id, member)
  std::vector<int> uid, seg;                  // the ids in ascending order; obs[seg[u], seg[u + 1]) holds uid[u]

  int find(int id) const {
    const size_t u = (size_t)(std::lower_bound(uid.begin(), uid.end(), id) - uid.begin());
    return u < uid.size() && uid[u] == id ? (int)u : -1;
  }
  // rows[m] / octs[m]: n[m] entries.  0, or -1 (an id twice in a row, too many members) with the previous index in place
  int build(int nm, const int* n, const int* const* rows, const int* const* octs) {
    if (nm < 0 || nm > CMS_COVIS_MAX_MEMBERS) return -1;
    std::vector<Obs> o;
    for (int m = 0; m < nm; ++m)
      for (int f = 0; f < n[m]; ++f)
        if (rows[m][f] >= 0) o.push_back(Obs{rows[m][f], m, f, octs[m][f]});
    std::sort(o.begin(), o.end(), [](const Obs& a, const Obs& b) { return a.id != b.id ? a.id < b.id : a.member != b.member ? a.member < b.member : a.feat < b.feat; });
    for (size_t i = 1; i < o.size(); ++i) if (o[i].id == o[i - 1].id && o[i].member == o[i - 1].member) return -1;
    n_members = nm;
    mp.assign((size_t)nm, std::vector<int>()); oct.assign((size_t)nm, std::vector<int>());
    for (int m = 0; m < nm; ++m) { mp[(size_t)m].assign(rows[m], rows[m] + n[m]); oct[(size_t)m].assign(octs[m], octs[m] + n[m]); }
    obs.swap(o);
    uid.clear(); seg.clear();
    for (size_t i = 0; i < obs.size(); ++i)
      if (i == 0 || obs[i].id != obs[i - 1].id) { uid.push_back(obs[i].id); seg.push_back((int)i); }
    seg.push_back((int)obs.size());
    return 0;
  }
  // keyframeCounter (Tracking.cpp:885-901): votes njobs x n_members
  int votes(int njobs, const int* id_off, const int* ids, int* out) const {
    for (int j = 0; j < njobs; ++j) for (int q = id_off[j]; q < id_off[j + 1]; ++q) if (ids[q] < 0) return -1;
    std::fill(out, out + (size_t)njobs * (size_t)n_members, 0);
    for (int j = 0; j < njobs; ++j)
      for (int q = id_off[j]; q < id_off[j + 1]; ++q) {
        const int u = find(ids[q]);
        if (u < 0) continue;
        for (int e = seg[(size_t)u]; e < seg[(size_t)u + 1]; ++e) ++out[(size_t)j * (size_t)n_members + (size_t)obs[(size_t)e].member];
      }
    return 0;
  }
  // KFcounter and the ordered list (KeyFrame.cpp:317-394)
  int connections(int njobs, const int* job_member, int th, int* weights, int* order, int* n_connected) const {
    for (int j = 0; j < njobs; ++j) if (job_member[j] < 0 || job_member[j] >= n_members) return -1;
    const size_t M = (size_t)n_members;
    for (int j = 0; j < njobs; ++j) {
      int* w = weights + (size_t)j * M;
      int* ord = order + (size_t)j * M;
      std::fill(w, w + M, 0); std::fill(ord, ord + M, -1);
      const int m0 = job_member[j];
      for (int id : mp[(size_t)m0]) {
        if (id < 0) continue;
        const int u = find(id);
        for (int e = seg[(size_t)u]; e < seg[(size_t)u + 1]; ++e) if (obs[(size_t)e].member != m0) ++w[obs[(size_t)e].member];
      }
      std::vector<int> c;
      int best = -1;
      for (int m = 0; m < n_members; ++m) {
        if (w[m] > 0 && (best < 0 || w[m] > w[best])) best = m;
        if (w[m] > 0 && w[m] >= th) c.push_back(m);
      }
      if (c.empty() && best >= 0) c.push_back(best);
      std::sort(c.begin(), c.end(), [&](int a, int b) { return cms_covis_before(w[a], a, w[b], b); });
      std::copy(c.begin(), c.end(), ord);
      n_connected[j] = (int)c.size();
    }
    return 0;
  }
  // the counters of KeyFrameCulling (LocalMapping.cpp:569-618) with what SetBadFlag does to the later candidates of the chain
  int culling(int n_chains, const int* chain_off, const int* job_member, const uint8_t* erasable, int th_obs, int* n_mps, int* n_redundant, uint8_t* redundant) const {
    if (th_obs < 0) return -1;
    for (int c = 0; c < n_chains; ++c) {
      if (chain_off[c + 1] < chain_off[c]) return -1;
      std::vector<uint8_t> seen((size_t)n_members, 0);
      for (int j = chain_off[c]; j < chain_off[c + 1]; ++j) {
        if (job_member[j] < 0 || job_member[j] >= n_members || seen[(size_t)job_member[j]]) return -1;
        seen[(size_t)job_member[j]] = 1;
      }
    }
    for (int c = 0; c < n_chains; ++c) {
      std::vector<int> cnt(uid.size());
      for (size_t u = 0; u < uid.size(); ++u) cnt[u] = seg[u + 1] - seg[u];
      std::vector<uint8_t> bad(uid.size(), 0), removed((size_t)n_members, 0);
      for (int j = chain_off[c]; j < chain_off[c + 1]; ++j) {
        const int m0 = job_member[j];
        const std::vector<int>& row = mp[(size_t)m0];
        int nm = 0, nr = 0;
        for (size_t f = 0; f < row.size(); ++f) {
          if (row[f] < 0) continue;
          const int u = find(row[f]);
          if (bad[(size_t)u]) continue;
          ++nm;
          if (!(cnt[(size_t)u] > th_obs)) continue;
          int n_obs = 0;
          for (int e = seg[(size_t)u]; e < seg[(size_t)u + 1] && n_obs < th_obs; ++e) {
            const Obs& o = obs[(size_t)e];
            if (o.member == m0 || removed[(size_t)o.member]) continue;
            if (cms_covis_octave_ok(o.octave, oct[(size_t)m0][f])) ++n_obs;
          }
          if (n_obs >= th_obs) ++nr;
        }
        n_mps[j] = nm; n_redundant[j] = nr; redundant[j] = cms_covis_redundant(nr, nm) ? 1 : 0;
        if (redundant[j] && erasable[j]) {      // KeyFrame::SetBadFlag (KeyFrame.cpp:494-496) -> MapPoint::EraseObservation (MapPoint.cpp:115-136)
          removed[(size_t)m0] = 1;
          for (int id : row) {
            if (id < 0) continue;
            const int u = find(id);
            if (bad[(size_t)u]) continue;
            if (cms_covis_point_dies(--cnt[(size_t)u])) bad[(size_t)u] = 1;
          }
        }
      }
    }
    return 0;
  }
  // mvpLocalMapPoints (Tracking.cpp:857-877) as ids; 0, -1, or -4 (CMS_ERR_OVERFLOW: n_out says how many, the first cap are written)
  int local_points(int njobs, const int* kf_off, const int* kf_members, int cap, int* ids_out, int* n_out) const {
    if (cap < 0) return -1;
    for (int j = 0; j < njobs; ++j) {
      if (kf_off[j + 1] < kf_off[j]) return -1;
      std::vector<uint8_t> seen((size_t)n_members, 0);
      for (int q = kf_off[j]; q < kf_off[j + 1]; ++q) {
        if (kf_members[q] < 0 || kf_members[q] >= n_members || seen[(size_t)kf_members[q]]) return -1;
        seen[(size_t)kf_members[q]] = 1;
      }
    }
    bool overflow = false;
    for (int j = 0; j < njobs; ++j) {
      std::vector<uint8_t> taken(uid.size(), 0);
      int n = 0;
      for (int q = kf_off[j]; q < kf_off[j + 1]; ++q)
        for (int id : mp[(size_t)kf_members[q]]) {
          if (id < 0) continue;
          const int u = find(id);
          if (taken[(size_t)u]) continue;
          taken[(size_t)u] = 1;
          if (n < cap) ids_out[(size_t)j * (size_t)cap + (size_t)n] = id;
          ++n;
        }
      n_out[j] = n;
      overflow = overflow || n > cap;
    }
    return overflow ? -4 : 0;
  }
};

// The store's stand-in of the host build: slots with an mp row and an octave row, what cms_kfstore_put / update / update_map_points keep per slot
struct CmsCovisHostStore {
  struct Slot { bool used = false; std::vector<int> mp, oct; };
  std::vector<Slot> slots;
  int max_features = 0, max_members = 0;
  CmsCovisHost index;
  CmsCovisHostStore(int max_keyframes, int max_feat, int max_mem) : slots((size_t)max_keyframes), max_features(max_feat), max_members(max_mem) {}
  bool slot_ok(int s) const { return s >= 0 && (size_t)s < slots.size(); }
  int put(int s, int n, const int* mp, const int* oct) {
    if (!slot_ok(s) || n < 0 || n > max_features || (n > 0 && (!mp || !oct))) return -1;
    Slot& e = slots[(size_t)s];
    e.used = true; e.mp.assign(mp, mp + n); e.oct.assign(oct, oct + n);
    return 0;
  }
  // all triples of the call or none
  int update_map_points(int n, const int* slot, const int* feat, const int* mp) {
    std::vector<unsigned long long> key;
    for (int i = 0; i < n; ++i) {
      if (!slot_ok(slot[i]) || !slots[(size_t)slot[i]].used || feat[i] < 0 || (size_t)feat[i] >= slots[(size_t)slot[i]].mp.size() || mp[i] < -1 || mp[i] > CMS_COVIS_MAX_ID) return -1;
      key.push_back(((unsigned long long)(unsigned)slot[i] << 32) | (unsigned)feat[i]);
    }
    std::sort(key.begin(), key.end());
    for (size_t i = 1; i < key.size(); ++i) if (key[i] == key[i - 1]) return -1;
    for (int i = 0; i < n; ++i) slots[(size_t)slot[i]].mp[(size_t)feat[i]] = mp[i];
    return 0;
  }
  // 0, -1 (an empty slot, a slot twice, an id twice in a row) or -3 (CMS_ERR_UNSUPPORTED: more than 16 384 members)
  int build(int nm, const int* member_slots) {
    if (nm < 0 || (nm > 0 && !member_slots)) return -1;
    if (nm > CMS_COVIS_MAX_MEMBERS) return -3;
    if (nm > max_members) return -1;
    std::vector<uint8_t> seen(slots.size(), 0);
    std::vector<int> n((size_t)nm);
    std::vector<const int*> rows((size_t)nm), octs((size_t)nm);
    for (int m = 0; m < nm; ++m) {
      const int s = member_slots[m];
      if (!slot_ok(s) || !slots[(size_t)s].used || seen[(size_t)s]) return -1;
      seen[(size_t)s] = 1;
      n[(size_t)m] = (int)slots[(size_t)s].mp.size(); rows[(size_t)m] = slots[(size_t)s].mp.data(); octs[(size_t)m] = slots[(size_t)s].oct.data();
    }
    return index.build(nm, n.data(), rows.data(), octs.data());
  }
};
#endif
