// Batch-structure cache: what a KFAC accumulate derives from the graph and a batch's node ids alone (lgnn_internal.h,
// BatchEntry).  Host code only -- the lists are built by the kernels of kfac_top.hip / paths.hip into the workspace exactly as
// without the cache, and copied into an entry of their exact size the second time a tag is seen.
//
// The training loop of the reference builds its loader once (gnn/marglik_training.py:125-127, shuffle=False) and calls
// la.fit(train_loader) again and again while the weights move: the batches, and with them these lists, repeat.
#include "lgnn_internal.h"

#include <algorithm>
#include <cstdlib>

namespace lgnn {

namespace {

constexpr size_t kSeenMax = 256;  // tags remembered after one sighting (8 bytes each)

// reset the entry, keep tag and M (its arrays free themselves; hipFree waits for the device: no kernel in flight still reads them)
void free_entry_memory(BatchEntry* e) {
  const uint64_t tag = e->tag;
  const int64_t M = e->M;
  *e = BatchEntry{};
  e->tag = tag;
  e->M = M;
}

void remove_entry(lgnn_ctx* h, BatchEntry* e) {
  BatchCache& c = h->bcache;
  c.bytes -= e->bytes;
  c.entries.erase(std::find(c.entries.begin(), c.entries.end(), e));
  delete e;
}

// room for `add` more bytes of entry `e`: the least recently used other entries go first; false if `e` alone is too large
bool make_room(lgnn_ctx* h, BatchEntry* e, size_t add, size_t budget) {
  BatchCache& c = h->bcache;
  if (e->bytes + add > budget) return false;
  while (c.bytes + add > budget) {
    BatchEntry* lru = nullptr;
    for (BatchEntry* o : c.entries)
      if (o != e && o->bytes > 0 && (!lru || o->last_use < lru->last_use)) lru = o;
    if (!lru) return false;
    remove_entry(h, lru);
  }
  return true;
}

// (exact size, not DevBuf::reserve: no 256-byte floor, and a failure only refuses the entry -- the HIP error is cleared and
// no message is left for the caller)
template <class T>
int alloc_copy(DevArray<T>& dst, const void* src, size_t count, hipStream_t s) {
  dst = {};
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  if (hipMalloc(&dst.buf.p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    dst.buf.p = nullptr;
    return 1;
  }
  dst.buf.bytes = bytes;
  if (count > 0) LGNN_HIP_CHECK(hipMemcpyAsync(dst.buf.p, src, count * sizeof(T), hipMemcpyDeviceToDevice, s));
  return 0;
}

// an entry that could not be kept (over the budget, out of memory): its memory goes, the tag stays known as "not cached"
void refuse(lgnn_ctx* h, BatchEntry* e) {
  h->bcache.bytes -= e->bytes;
  free_entry_memory(e);
  e->refused = true;
}

}  // namespace

// LGNN_BATCH_CACHE_MB, read per call: the cache's byte budget (0: off).  Default 2 GiB: the ten batches of the arxiv shape
// take 0.27 GB, ten batches of a graph ten times as dense still fit, and it is small against the 32 GB workspace limit.
size_t batch_cache_budget() {
  const char* e = getenv("LGNN_BATCH_CACHE_MB");
  const long long mb = e ? atoll(e) : 2048;
  return mb <= 0 ? 0 : size_t(mb) << 20;
}

void batch_cache_clear(lgnn_ctx* h) {
  BatchCache& c = h->bcache;
  for (BatchEntry* e : c.entries) delete e;
  c.entries.clear();
  c.seen.clear();
  c.bytes = 0;
}

void batch_cache_drop_tag(lgnn_ctx* h, uint64_t tag) {
  BatchCache& c = h->bcache;
  for (BatchEntry* e : c.entries)
    if (e->tag == tag) { remove_entry(h, e); break; }
  c.seen.erase(std::remove(c.seen.begin(), c.seen.end(), tag), c.seen.end());
}

// The entry of (tag, M), or null: no tag, cache off, first sighting (the tag is remembered), or a batch that was refused.
// A tag seen for the second time gets an empty entry (with a copy of the ids), which the caller's build steps fill.
int batch_cache_lookup(lgnn_ctx* h, uint64_t tag, const int64_t* idx, int64_t M, BatchEntry** out, hipStream_t s) {
  *out = nullptr;
  BatchCache& c = h->bcache;
  if (tag == 0) return 0;
  const size_t budget = batch_cache_budget();
  if (budget == 0) {
    if (!c.entries.empty() || !c.seen.empty()) batch_cache_clear(h);
    return 0;
  }
  while (c.bytes > budget) {  // (the budget is read per call: it may have shrunk)
    BatchEntry* lru = nullptr;
    for (BatchEntry* o : c.entries)
      if (o->bytes > 0 && (!lru || o->last_use < lru->last_use)) lru = o;
    if (!lru) break;
    remove_entry(h, lru);
  }
  for (BatchEntry* e : c.entries)
    if (e->tag == tag) {
      if (e->M != M) { remove_entry(h, e); break; }  // (a tag names one batch: another length is another batch)
      if (e->refused) return 0;
      e->last_use = ++c.clock;
      *out = e;
      return 0;
    }
  auto it = std::find(c.seen.begin(), c.seen.end(), tag);
  if (it == c.seen.end()) {
    if (c.seen.size() >= kSeenMax) c.seen.erase(c.seen.begin());
    c.seen.push_back(tag);
    return 0;
  }
  c.seen.erase(it);
  BatchEntry* e = new (std::nothrow) BatchEntry();
  if (!e) return 0;
  e->tag = tag;
  e->M = M;
  e->last_use = ++c.clock;
  c.entries.push_back(e);
  const size_t add = size_t(M) * 8;
  if (!make_room(h, e, add, budget) || alloc_copy(e->ids, idx, size_t(M), s) != 0) { refuse(h, e); return 0; }
  e->bytes += add;
  c.bytes += add;
  *out = e;
  return 0;
}

// Copy the active-row flags / list / count the caller has just built in the workspace into the entry.  Synchronises the
// stream once (the list's length has to reach the host to size the copy).
int batch_cache_store_active(lgnn_ctx* h, BatchEntry* e, hipStream_t s) {
  if (e->has_act || e->refused) return 0;
  const int64_t N = h->N;
  int32_t n = 0;
  LGNN_HIP_CHECK(hipMemcpyAsync(&n, h->ws.act_count.p, 4, hipMemcpyDeviceToHost, s));
  LGNN_HIP_CHECK(hipStreamSynchronize(s));
  LGNN_REQUIRE(n >= 0 && n <= N, "internal: active-row count out of range");
  const size_t add = size_t(N) + size_t(std::max(n, 1)) * 4 + 4;
  if (!make_room(h, e, add, batch_cache_budget()) || alloc_copy(e->active, h->ws.active.p, size_t(N), s) != 0 ||
      alloc_copy(e->act_list, h->ws.act_list.p, size_t(n), s) != 0 ||
      alloc_copy(e->act_count, h->ws.act_count.p, 1, s) != 0) {
    refuse(h, e);
    return 0;
  }
  e->bytes += add;
  h->bcache.bytes += add;
  e->has_act = true;
  return 0;
}

// The same for the two-hop path list, R (the top-layer tiles read it on every accumulate, the overflow route where it can be
// reached) and the node list of a short batch when the caller built one over all N nodes.  Synchronises the stream once.
int batch_cache_store_paths(lgnn_ctx* h, BatchEntry* e, int64_t cap, bool have_nodes, hipStream_t s) {
  if (e->has_paths || e->refused) return 0;
  const int64_t N = h->N;
  Workspace& ws = h->ws;
  int32_t cnt[3] = {0, 0, 0};  // paths, entries of R, nodes with a path
  LGNN_HIP_CHECK(hipMemcpyAsync(&cnt[0], ws.path_pptr.as<int32_t>() + N, 4, hipMemcpyDeviceToHost, s));
  LGNN_HIP_CHECK(hipMemcpyAsync(&cnt[1], ws.path_rptr.as<int32_t>() + N, 4, hipMemcpyDeviceToHost, s));
  if (have_nodes) LGNN_HIP_CHECK(hipMemcpyAsync(&cnt[2], ws.path_nnodes.p, 4, hipMemcpyDeviceToHost, s));
  LGNN_HIP_CHECK(hipStreamSynchronize(s));
  // (a list longer than its capacity was counted, not filled: the fused kernel returns at once and the overflow route runs)
  const size_t np = (cnt[0] >= 0 && int64_t(cnt[0]) <= cap) ? size_t(cnt[0]) : 0;
  LGNN_REQUIRE(cnt[1] >= 0 && int64_t(cnt[1]) <= std::max<int64_t>(h->nnz, 1) && cnt[2] >= 0 && cnt[2] <= N,
               "internal: path structure counts out of range");
  const size_t nr = size_t(cnt[1]), nn = size_t(cnt[2]);
  size_t add = size_t(N + 2) * 4 + std::max<size_t>(np, 1) * 12;  // (pptr: N + 1 pointers and the list's wsum, paths.hip)
  add += size_t(N + 1) * 4 + std::max<size_t>(nr, 1) * 8;
  if (have_nodes) add += std::max<size_t>(nn, 1) * 4 + 4;
  bool ok = make_room(h, e, add, batch_cache_budget());
  ok = ok && alloc_copy(e->pptr, ws.path_pptr.p, size_t(N + 2), s) == 0 && alloc_copy(e->pm, ws.path_pm.p, np, s) == 0 &&
       alloc_copy(e->pv, ws.path_pv.p, np, s) == 0 && alloc_copy(e->pw, ws.path_pw.p, np, s) == 0;
  if (ok)
    ok = alloc_copy(e->rptr, ws.path_rptr.p, size_t(N + 1), s) == 0 && alloc_copy(e->r_m, ws.path_rm.p, nr, s) == 0 &&
         alloc_copy(e->r_w, ws.path_rw.p, nr, s) == 0;
  if (ok && have_nodes)
    ok = alloc_copy(e->nodes, ws.path_nodes.p, nn, s) == 0 && alloc_copy(e->nnodes, ws.path_nnodes.p, 1, s) == 0;
  if (!ok) { refuse(h, e); return 0; }
  e->bytes += add;
  h->bcache.bytes += add;
  e->path_bytes = add;
  e->cap = cap;
  e->has_nodes = have_nodes;
  e->has_paths = true;
  return 0;
}

// The top layer's term lists (toppairs.hip), which the caller has just built in the workspace from the entry's R (or from
// the workspace's R the entry's was copied from): part of the path structure.  Synchronises the stream once.  The caller may be
// reading the entry's R and path list in this very call: lists that cannot be kept (over the budget, out of memory) leave the
// rest of the entry as it is -- only the pair part stays out, for good (pairs_refused), and is built per call.
int batch_cache_store_pairs(lgnn_ctx* h, BatchEntry* e, hipStream_t s) {
  if (e->has_pairs || e->pairs_refused || e->refused || !e->has_paths) return 0;
  const int64_t N = h->N;
  Workspace& ws = h->ws;
  int32_t np = 0;
  LGNN_HIP_CHECK(hipMemcpyAsync(&np, ws.pair_ptr.as<int32_t>() + N, 4, hipMemcpyDeviceToHost, s));
  LGNN_HIP_CHECK(hipStreamSynchronize(s));
  LGNN_REQUIRE(np >= 0 && size_t(np) * 4 <= ws.pair_m.bytes, "internal: pair count out of range");
  const size_t M = size_t(e->M), add = M * 4 + std::max<size_t>(size_t(np), 1) * 12 + 4;
  const bool ok = make_room(h, e, add, batch_cache_budget()) && alloc_copy(e->pair_s, ws.pair_s.p, M, s) == 0 &&
                  alloc_copy(e->pair_m, ws.pair_m.p, size_t(np), s) == 0 && alloc_copy(e->pair_m2, ws.pair_m2.p, size_t(np), s) == 0 &&
                  alloc_copy(e->pair_w, ws.pair_w.p, size_t(np), s) == 0 &&
                  alloc_copy(e->pair_n, ws.pair_ptr.as<int32_t>() + N, 1, s) == 0;
  if (!ok) {
    e->pair_s = {}; e->pair_m = {}; e->pair_m2 = {}; e->pair_w = {}; e->pair_n = {};
    e->pairs_refused = true;
    return 0;
  }
  e->bytes += add;
  h->bcache.bytes += add;
  e->path_bytes += add;
  e->has_pairs = true;
  return 0;
}

// another list capacity (LGNN_PATH_LIST_CAP): the path part is built again
void batch_cache_drop_paths(lgnn_ctx* h, BatchEntry* e) {
  if (!e->has_paths) return;
  e->pair_s = {}; e->pair_m = {}; e->pair_m2 = {}; e->pair_w = {}; e->pair_n = {};
  e->has_pairs = e->pairs_refused = false;
  e->pptr = {}; e->pm = {}; e->pv = {}; e->pw = {}; e->nodes = {}; e->nnodes = {}; e->rptr = {}; e->r_m = {}; e->r_w = {};
  e->has_paths = e->has_nodes = false;
  h->bcache.bytes -= e->path_bytes;
  e->bytes -= e->path_bytes;
  e->path_bytes = 0;
}

}  // namespace lgnn

using namespace lgnn;

extern "C" int lgnn_kfac_batch_tag(lgnn_ctx* h, uint64_t tag) {
  if (!h) { set_error("null context"); return 2; }
  h->bcache.pending_tag = tag;
  return 0;
}

extern "C" int lgnn_batch_cache_drop(lgnn_ctx* h, uint64_t tag) {
  if (!h) { set_error("null context"); return 2; }
  if (tag == 0) batch_cache_clear(h);
  else batch_cache_drop_tag(h, tag);
  return 0;
}

extern "C" int lgnn_batch_cache_stats(const lgnn_ctx* h, int64_t* out) {
  if (!h || !out) { set_error("null argument"); return 2; }
  const BatchCache& c = h->bcache;
  int64_t n = 0;
  for (const BatchEntry* e : c.entries) n += e->bytes > 0 ? 1 : 0;
  out[0] = n; out[1] = int64_t(c.bytes); out[2] = c.hits; out[3] = c.misses; out[4] = c.builds;
  return 0;
}
