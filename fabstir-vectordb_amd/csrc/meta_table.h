// meta_table.h — metadata columns of the C ABI (include/fvdb.h, "metadata columns"): the table of
// typed columns in HBM, its mutations, and the evaluation of a filter program over it.  Included at the end of
// fvdb_hip.cpp.  Everything a kernel indexes with is checked here first: slots against the table, columns and constants
// against the program's own tables, and an ARRAY cell's offset and length are written by this file, never by the caller.
#pragma once
#include "kernels_meta.h"

struct MetaCol {
  DBuf tag, val;               // [cap] of the table
  DBuf etag, eval;             // [e_cap]
  uint64_t e_used = 0, e_live = 0, e_cap = 0;
  std::vector<uint32_t> alen;  // [slots]: length of the slot's ARRAY cell (0: not an array), to count what a rewrite leaves dead
};

struct fvdb_meta {
  fvdb_ctx* ctx = nullptr;
  std::mutex mu;
  uint64_t slots = 0, cap = 0, present = 0;
  DBuf ids, pres;               // [cap]
  std::vector<uint8_t> h_pres;  // host copy of pres, to keep `present` counted
  std::vector<MetaCol> cols;
  DBuf coltab;                  // MetaColumn[cols], uploaded when a column appeared or moved
  bool coltab_dirty = true;
  DBuf idx_id, idx_slot;        // id -> slot index (kernels_meta.h): [idx_cells] id words and slot words
  uint64_t idx_cells = 0;       // a power of two >= 2 * slots once built
  bool idx_dirty = true;        // set_rows has run since the last build
  DBuf prog;                    // constants' keys, instructions, constants' tags of the evaluation in flight
  DBuf ballots, counts, totals, out_ids, out_unknown, out_rank;
  uint64_t n_match = 0, n_unknown = 0;
  bool have_result = false;
};

namespace {

// room for `want` slots in every per-slot array, contents kept, the new tail zero (MISSING, not present).  A failure
// partway leaves the arrays grown so far at the new size and t->cap as it was: every array then still holds at least
// t->cap slots with their contents, and the next call grows all of them again.
int meta_reserve(fvdb_meta* t, uint64_t want) {
  fvdb_ctx* ctx = t->ctx;
  if (want <= t->cap) return FVDB_OK;
  const uint64_t cap = std::max<uint64_t>({want, t->cap * 2, 1024});
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, grow_keeping(t->ids, cap * 8, t->slots * 8, true, st));
  HIPCHK(ctx, grow_keeping(t->pres, cap, t->slots, true, st));
  for (MetaCol& c : t->cols) {
    HIPCHK(ctx, grow_keeping(c.tag, cap, t->slots, true, st));
    HIPCHK(ctx, grow_keeping(c.val, cap * 8, t->slots * 8, true, st));
  }
  t->coltab_dirty = true;
  t->have_result = false;  // the result buffers are sized with the table
  t->cap = cap;
  return FVDB_OK;
}

bool strictly_ascending_below(const uint32_t* slots, uint64_t n, uint64_t limit) {
  for (uint64_t i = 0; i < n; ++i)
    if (slots[i] >= limit || (i && slots[i] <= slots[i - 1])) return false;
  return true;
}

// FVDB_E_INVALID / FVDB_E_UNSUPPORTED with a message, or FVDB_OK: every index the kernel will follow is in range
int meta_check_program(fvdb_meta* t, const uint32_t* instrs, uint32_t n_instrs, const uint32_t* ctag, const uint64_t* ckey, uint32_t n_consts) {
  fvdb_ctx* ctx = t->ctx;
  if (n_instrs > FVDB_META_MAX_PROGRAM) FAIL(ctx, FVDB_E_UNSUPPORTED, "filter program longer than FVDB_META_MAX_PROGRAM");
  if (n_consts > FVDB_META_MAX_CONSTS) FAIL(ctx, FVDB_E_UNSUPPORTED, "filter program with more than FVDB_META_MAX_CONSTS constants");
  if (n_instrs == 0 || !instrs) FAIL(ctx, FVDB_E_INVALID, "empty filter program");
  if (n_consts && (!ctag || !ckey)) FAIL(ctx, FVDB_E_INVALID, "null constant pool");
  for (uint32_t i = 0; i < n_consts; ++i)
    if (!((ctag[i] >= FVDB_META_NULL && ctag[i] <= FVDB_META_STRING) || ctag[i] == FVDB_META_COMPLEX || ctag[i] == FVDB_META_NEVER))
      FAIL(ctx, FVDB_E_INVALID, "constant with an unknown tag");
  uint32_t sp = 0;
  for (uint32_t pc = 0; pc < n_instrs; ++pc) {
    const uint32_t* in = instrs + 4 * (size_t)pc;
    const uint32_t op = in[0] & 0xFFu, flags = in[0] >> 8;
    if (op == FVDB_META_OP_AND || op == FVDB_META_OP_OR) {
      if (flags) FAIL(ctx, FVDB_E_INVALID, "AND / OR with flags");
      if (in[1] > FVDB_META_MAX_STACK) FAIL(ctx, FVDB_E_UNSUPPORTED, "AND / OR of more than FVDB_META_MAX_STACK operands");
      if (in[1] > sp) FAIL(ctx, FVDB_E_INVALID, "filter program: stack underflow");
      sp -= in[1];
    } else if (op == FVDB_META_OP_EQUALS || op == FVDB_META_OP_IN || op == FVDB_META_OP_RANGE) {
      if (in[1] >= t->cols.size()) FAIL(ctx, FVDB_E_INVALID, "filter program: column out of range");
      const uint64_t first = in[2], n = op == FVDB_META_OP_IN ? in[3] : (op == FVDB_META_OP_RANGE ? 2 : 1);
      if (first + n > n_consts) FAIL(ctx, FVDB_E_INVALID, "filter program: constant out of range");
      if (op == FVDB_META_OP_EQUALS && flags) FAIL(ctx, FVDB_E_INVALID, "EQUALS with flags");
      if (op == FVDB_META_OP_IN) {
        if (flags > 3u) FAIL(ctx, FVDB_E_INVALID, "IN with unknown flags");
        for (uint64_t i = first; i < first + n; ++i) {
          if (ctag[i] > FVDB_META_STRING) FAIL(ctx, FVDB_E_INVALID, "IN: a COMPLEX or NEVER constant in the sorted list");
          if (i > first && !(ctag[i - 1] < ctag[i] || (ctag[i - 1] == ctag[i] && ckey[i - 1] < ckey[i])))
            FAIL(ctx, FVDB_E_INVALID, "IN: constants not sorted by (tag, key)");
        }
      }
      if (op == FVDB_META_OP_RANGE) {
        if (flags > 15u) FAIL(ctx, FVDB_E_INVALID, "RANGE with unknown flags");
        if (ctag[first] != FVDB_META_FLOAT || ctag[first + 1] != FVDB_META_FLOAT) FAIL(ctx, FVDB_E_INVALID, "RANGE: bounds must be FLOAT constants");
      }
    } else {
      FAIL(ctx, FVDB_E_INVALID, "filter program: unknown op");
    }
    if (sp >= FVDB_META_MAX_STACK) FAIL(ctx, FVDB_E_UNSUPPORTED, "filter program deeper than FVDB_META_MAX_STACK");
    sp += 1;
  }
  if (sp != 1) FAIL(ctx, FVDB_E_INVALID, "filter program must leave exactly one result");
  return FVDB_OK;
}

}  // namespace

extern "C" {

int fvdb_meta_create(fvdb_ctx* ctx, fvdb_meta** out) {
  if (!ctx || !out) return FVDB_E_INVALID;
  *out = nullptr;
  fvdb_meta* t = new (std::nothrow) fvdb_meta();
  if (!t) return FVDB_E_OOM;
  t->ctx = ctx;
  *out = t;
  return FVDB_OK;
}

void fvdb_meta_destroy(fvdb_meta* t) {
  if (!t) return;
  (void)hipSetDevice(t->ctx->device);
  (void)hipStreamSynchronize(t->ctx->stream);
  delete t;
}

int fvdb_meta_info(fvdb_meta* t, fvdb_meta_info_t* out) {
  if (!t || !out) return FVDB_E_INVALID;
  std::lock_guard<std::mutex> lk(t->mu);
  out->slots = t->slots;
  out->present = t->present;
  out->columns = t->cols.size();
  out->live_elements = out->dead_elements = 0;
  uint64_t bytes = t->ids.cap + t->pres.cap + t->idx_id.cap + t->idx_slot.cap + t->coltab.cap + t->prog.cap + t->ballots.cap + t->counts.cap + t->totals.cap +
                   t->out_ids.cap + t->out_unknown.cap + t->out_rank.cap;
  for (const MetaCol& c : t->cols) {
    out->live_elements += c.e_live;
    out->dead_elements += c.e_used - c.e_live;
    bytes += c.tag.cap + c.val.cap + c.etag.cap + c.eval.cap;
  }
  out->hbm_bytes = bytes;
  return FVDB_OK;
}

int fvdb_meta_set_rows(fvdb_meta* t, uint64_t first, uint64_t n, const uint64_t* ids, const uint8_t* present) {
  if (!t) return FVDB_E_INVALID;
  fvdb_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(t->mu);
  if (n && (!ids || !present)) FAIL(ctx, FVDB_E_INVALID, "metadata rows: null argument");
  if (first > t->slots) FAIL(ctx, FVDB_E_INVALID, "metadata rows: a run must start inside the table or at its end");
  if (first + n < first || first + n >= (1ull << 32)) FAIL(ctx, FVDB_E_UNSUPPORTED, "metadata table of 2^32 slots or more");
  if (n == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = meta_reserve(t, first + n)) return rc;
  t->idx_dirty = true;  // the id index is rebuilt by the next key lookup
  HIPCHK(ctx, hipMemcpyAsync(t->ids.as<uint64_t>() + first, ids, n * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(t->pres.as<uint8_t>() + first, present, n, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the caller's arrays are its own again
  if (first + n > t->slots) {
    t->slots = first + n;
    t->h_pres.resize(t->slots, 0);
    for (MetaCol& c : t->cols) c.alen.resize(t->slots, 0);
  }
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t p = present[i] ? 1 : 0;
    t->present += (uint64_t)p - t->h_pres[first + i];
    t->h_pres[first + i] = p;
  }
  return FVDB_OK;
}

int fvdb_meta_set_present(fvdb_meta* t, const uint32_t* slots, const uint8_t* present, uint64_t n) {
  if (!t) return FVDB_E_INVALID;
  fvdb_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(t->mu);
  if (n && (!slots || !present)) FAIL(ctx, FVDB_E_INVALID, "metadata presence: null argument");
  if (!strictly_ascending_below(slots, n, t->slots)) FAIL(ctx, FVDB_E_INVALID, "metadata presence: slots must be ascending and inside the table");
  if (n == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DBuf d_slots, d_bytes;
  if (int rc = upload_temp(ctx, d_slots, slots, n * 4)) return rc;
  if (int rc = upload_temp(ctx, d_bytes, present, n)) return rc;
  hipLaunchKernelGGL(meta_scatter_bytes_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, (const uint32_t*)d_slots.p,
                     (const uint8_t*)d_bytes.p, n, t->pres.as<uint8_t>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (uint64_t i = 0; i < n; ++i) {
    const uint8_t p = present[i] ? 1 : 0;
    t->present += (uint64_t)p - t->h_pres[slots[i]];
    t->h_pres[slots[i]] = p;
  }
  return FVDB_OK;
}

int fvdb_meta_add_column(fvdb_meta* t, uint32_t* out_column) {
  if (!t || !out_column) return FVDB_E_INVALID;
  fvdb_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(t->mu);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  MetaCol c;
  const size_t cap = std::max<uint64_t>(t->cap, 1);
  HIPCHK(ctx, c.tag.exact(cap));
  HIPCHK(ctx, c.val.exact(cap * 8));
  HIPCHK(ctx, hipMemsetAsync(c.tag.p, 0, cap, ctx->stream));  // MISSING everywhere
  HIPCHK(ctx, hipMemsetAsync(c.val.p, 0, cap * 8, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  c.alen.assign(t->slots, 0);
  t->cols.push_back(std::move(c));
  t->coltab_dirty = true;
  *out_column = (uint32_t)(t->cols.size() - 1);
  return FVDB_OK;
}

int fvdb_meta_set_cells(fvdb_meta* t, uint32_t column, const uint32_t* slots, const uint8_t* tags, const uint64_t* vals, uint64_t n,
                        const uint8_t* elem_tags, const uint64_t* elem_vals, uint64_t n_elems) {
  if (!t) return FVDB_E_INVALID;
  fvdb_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(t->mu);
  if (column >= t->cols.size()) FAIL(ctx, FVDB_E_INVALID, "metadata cells: column out of range");
  if (n && (!slots || !tags || !vals)) FAIL(ctx, FVDB_E_INVALID, "metadata cells: null argument");
  if (n_elems && (!elem_tags || !elem_vals)) FAIL(ctx, FVDB_E_INVALID, "metadata cells: null element arrays");
  if (!strictly_ascending_below(slots, n, t->slots)) FAIL(ctx, FVDB_E_INVALID, "metadata cells: slots must be ascending and inside the table");
  MetaCol& c = t->cols[column];
  uint64_t need = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (tags[i] > FVDB_META_COMPLEX) FAIL(ctx, FVDB_E_INVALID, "metadata cells: unknown tag");
    if (tags[i] == FVDB_META_BOOL && vals[i] > 1) FAIL(ctx, FVDB_E_INVALID, "metadata cells: a BOOL payload must be 0 or 1");
    if (tags[i] == FVDB_META_ARRAY) {
      if (vals[i] > n_elems - need) FAIL(ctx, FVDB_E_INVALID, "metadata cells: ARRAY lengths exceed the elements given");
      need += vals[i];
    }
  }
  if (need != n_elems) FAIL(ctx, FVDB_E_INVALID, "metadata cells: elements given that no ARRAY cell takes");
  for (uint64_t i = 0; i < n_elems; ++i) {
    if (elem_tags[i] == FVDB_META_MISSING || elem_tags[i] == FVDB_META_ARRAY || elem_tags[i] > FVDB_META_COMPLEX)
      FAIL(ctx, FVDB_E_INVALID, "metadata cells: an element must be NULL, BOOL, INT, FLOAT, STRING or COMPLEX");
    if (elem_tags[i] == FVDB_META_BOOL && elem_vals[i] > 1) FAIL(ctx, FVDB_E_INVALID, "metadata cells: a BOOL payload must be 0 or 1");
  }
  if (c.e_used + n_elems >= (1ull << 32)) FAIL(ctx, FVDB_E_UNSUPPORTED, "metadata column of 2^32 elements or more");
  if (n == 0) return FVDB_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (c.e_used + n_elems > c.e_cap) {
    const uint64_t e_cap = std::max<uint64_t>({c.e_used + n_elems, c.e_cap * 2, 1024});
    HIPCHK(ctx, grow_keeping(c.etag, e_cap, c.e_used, true, ctx->stream));
    HIPCHK(ctx, grow_keeping(c.eval, e_cap * 8, c.e_used * 8, true, ctx->stream));
    c.e_cap = e_cap;
    t->coltab_dirty = true;
  }
  // the cells as the kernel reads them: an ARRAY's payload is where its elements went
  std::vector<uint64_t> payload(vals, vals + n);
  uint64_t at = c.e_used;
  for (uint64_t i = 0; i < n; ++i) {
    if (tags[i] == FVDB_META_ARRAY) {
      payload[i] = at | (vals[i] << 32);
      at += vals[i];
    } else if (tags[i] == FVDB_META_MISSING || tags[i] == FVDB_META_NULL || tags[i] == FVDB_META_COMPLEX) {
      payload[i] = 0;
    }
  }
  DBuf d_slots, d_tags, d_vals;
  if (int rc = upload_temp(ctx, d_slots, slots, n * 4)) return rc;
  if (int rc = upload_temp(ctx, d_tags, tags, n)) return rc;
  if (int rc = upload_temp(ctx, d_vals, payload.data(), n * 8)) return rc;
  if (n_elems) {
    HIPCHK(ctx, hipMemcpyAsync(c.etag.as<uint8_t>() + c.e_used, elem_tags, n_elems, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(c.eval.as<uint64_t>() + c.e_used, elem_vals, n_elems * 8, hipMemcpyHostToDevice, ctx->stream));
  }
  hipLaunchKernelGGL(meta_scatter_cells_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, (const uint32_t*)d_slots.p,
                     (const uint8_t*)d_tags.p, (const uint64_t*)d_vals.p, n, c.tag.as<uint8_t>(), c.val.as<uint64_t>());
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t len = tags[i] == FVDB_META_ARRAY ? (uint32_t)vals[i] : 0u;
    c.e_live += len;
    c.e_live -= c.alen[slots[i]];
    c.alen[slots[i]] = len;
  }
  c.e_used += n_elems;
  return FVDB_OK;
}

int fvdb_meta_eval(fvdb_meta* t, const uint32_t* instrs, uint32_t n_instrs, const uint32_t* const_tags, const uint64_t* const_keys,
                   uint32_t n_consts, uint64_t* out_matches, uint64_t* out_unknown) {
  if (!t) return FVDB_E_INVALID;
  fvdb_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(t->mu);
  if (!out_matches || !out_unknown) FAIL(ctx, FVDB_E_INVALID, "metadata eval: null argument");
  if (int rc = meta_check_program(t, instrs, n_instrs, const_tags, const_keys, n_consts)) return rc;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  t->have_result = false;
  *out_matches = *out_unknown = 0;
  if (t->slots == 0) {
    t->n_match = t->n_unknown = 0;
    t->have_result = true;
    return FVDB_OK;
  }
  const uint32_t slots = (uint32_t)t->slots, n_wg = cdiv(slots, 256);
  hipStream_t st = ctx->stream;
  if (t->coltab_dirty) {
    std::vector<MetaColumn> tab(t->cols.size());
    for (size_t i = 0; i < tab.size(); ++i)
      tab[i] = MetaColumn{t->cols[i].tag.as<uint8_t>(), t->cols[i].val.as<uint64_t>(), t->cols[i].etag.as<uint8_t>(), t->cols[i].eval.as<uint64_t>()};
    HIPCHK(ctx, t->coltab.ensure(std::max<size_t>(tab.size() * sizeof(MetaColumn), 8)));
    HIPCHK(ctx, hipMemcpyAsync(t->coltab.p, tab.data(), tab.size() * sizeof(MetaColumn), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    t->coltab_dirty = false;
  }
  // program block: keys (8-byte aligned), instructions (16-byte aligned), tags
  const size_t key_bytes = ((size_t)n_consts * 8 + 15) & ~(size_t)15, instr_bytes = (size_t)n_instrs * 16, tag_bytes = (size_t)n_consts * 4;
  HIPCHK(ctx, t->prog.ensure(key_bytes + instr_bytes + std::max<size_t>(tag_bytes, 4)));
  char* pb = (char*)t->prog.p;
  if (n_consts) HIPCHK(ctx, hipMemcpyAsync(pb, const_keys, (size_t)n_consts * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(pb + key_bytes, instrs, instr_bytes, hipMemcpyHostToDevice, st));
  if (n_consts) HIPCHK(ctx, hipMemcpyAsync(pb + key_bytes + instr_bytes, const_tags, tag_bytes, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, t->ballots.ensure((size_t)n_wg * 4 * 2 * 8));
  HIPCHK(ctx, t->counts.ensure((size_t)n_wg * 2 * 4));
  HIPCHK(ctx, t->totals.ensure(16));
  HIPCHK(ctx, t->out_ids.ensure(t->cap * 8));
  HIPCHK(ctx, t->out_unknown.ensure(t->cap * 4));
  HIPCHK(ctx, t->out_rank.ensure(t->cap * 4));
  MetaEvalArgs a{};
  a.present = t->pres.as<uint8_t>();
  a.cols = t->coltab.as<MetaColumn>();
  a.instr = (const uint4*)(pb + key_bytes);
  a.ctag = (const uint32_t*)(pb + key_bytes + instr_bytes);
  a.ckey = (const uint64_t*)pb;
  a.ballots = t->ballots.as<uint64_t>();
  a.cnt_match = t->counts.as<uint32_t>();
  a.cnt_unknown = t->counts.as<uint32_t>() + n_wg;
  a.slots = slots;
  a.n_instr = n_instrs;
  unsigned long long* totals = t->totals.as<unsigned long long>();
  hipLaunchKernelGGL(meta_eval_kernel, dim3(n_wg), dim3(256), 0, st, a);
  hipLaunchKernelGGL(block_excl_scan_kernel<unsigned long long>, dim3(1), dim3(1024), 0, st, a.cnt_match, n_wg, totals);
  hipLaunchKernelGGL(block_excl_scan_kernel<unsigned long long>, dim3(1), dim3(1024), 0, st, a.cnt_unknown, n_wg, totals + 1);
  hipLaunchKernelGGL(meta_write_kernel, dim3(n_wg), dim3(256), 0, st, t->ids.as<uint64_t>(), (const uint64_t*)a.ballots,
                     (const uint32_t*)a.cnt_match, (const uint32_t*)a.cnt_unknown, t->out_ids.as<uint64_t>(), t->out_unknown.as<uint32_t>(),
                     t->out_rank.as<uint32_t>());
  HIPCHK(ctx, hipGetLastError());
  unsigned long long h_tot[2] = {0, 0};
  HIPCHK(ctx, hipMemcpyAsync(h_tot, totals, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));  // also: the caller's program arrays are its own again
  t->n_match = h_tot[0];
  t->n_unknown = h_tot[1];
  t->have_result = true;
  *out_matches = t->n_match;
  *out_unknown = t->n_unknown;
  return FVDB_OK;
}

int fvdb_meta_eval_fetch(fvdb_meta* t, uint64_t* ids, uint32_t* unknown_slots, uint32_t* unknown_ranks) {
  if (!t) return FVDB_E_INVALID;
  fvdb_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(t->mu);
  if (!t->have_result) FAIL(ctx, FVDB_E_INVALID, "metadata eval: no result to fetch");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ids && t->n_match) HIPCHK(ctx, hipMemcpyAsync(ids, t->out_ids.p, t->n_match * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (unknown_slots && t->n_unknown)
    HIPCHK(ctx, hipMemcpyAsync(unknown_slots, t->out_unknown.p, t->n_unknown * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (unknown_ranks && t->n_unknown)
    HIPCHK(ctx, hipMemcpyAsync(unknown_ranks, t->out_rank.p, t->n_unknown * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return FVDB_OK;
}

int fvdb_meta_eval_dev(fvdb_meta* t, const uint64_t** ids_dev, const uint32_t** unknown_slots_dev, const uint32_t** unknown_ranks_dev,
                       uint64_t* out_matches, uint64_t* out_unknown) {
  if (!t) return FVDB_E_INVALID;
  std::lock_guard<std::mutex> lk(t->mu);
  if (!t->have_result) FAIL(t->ctx, FVDB_E_INVALID, "metadata eval: no result");
  if (ids_dev) *ids_dev = t->out_ids.as<uint64_t>();
  if (unknown_slots_dev) *unknown_slots_dev = t->out_unknown.as<uint32_t>();
  if (unknown_ranks_dev) *unknown_ranks_dev = t->out_rank.as<uint32_t>();
  if (out_matches) *out_matches = t->n_match;
  if (out_unknown) *out_unknown = t->n_unknown;
  return FVDB_OK;
}

// The keys of n candidate ids under one column: the id index is built here when set_rows has run
// since the last build, then one thread per id looks its slot up and reads presence and the cell as they are now.
int fvdb_group_keys_of_ids_dev(fvdb_meta* t, uint32_t column, const uint64_t* ids_dev, uint64_t n, uint8_t* out_tag_dev, uint64_t* out_key_dev) {
  if (!t) return FVDB_E_INVALID;
  fvdb_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(t->mu);
  if (column >= t->cols.size()) FAIL(ctx, FVDB_E_INVALID, "group keys: column out of range");
  if (n >= (1ull << 31)) FAIL(ctx, FVDB_E_UNSUPPORTED, "group keys: 2^31 ids or more in one call");
  if (n == 0) return FVDB_OK;
  if (!ids_dev || !out_tag_dev || !out_key_dev) FAIL(ctx, FVDB_E_INVALID, "group keys: null buffer");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const uint32_t slots = (uint32_t)t->slots;  // < 2^32: set_rows
  if (t->idx_dirty && slots) {
    uint64_t cells = 1024;
    while (cells < 2 * t->slots) cells <<= 1;  // <= 2^33 > 2 * slots; the mask below needs cells <= 2^32
    if (cells > (1ull << 32)) FAIL(ctx, FVDB_E_UNSUPPORTED, "group keys: a table of 2^31 slots or more");
    if (cells != t->idx_cells) {
      t->idx_cells = 0;
      HIPCHK(ctx, hipStreamSynchronize(st));  // a lookup enqueued earlier may still read the old arrays
      HIPCHK(ctx, t->idx_id.exact(cells * 8));
      HIPCHK(ctx, t->idx_slot.exact(cells * 4));
      t->idx_cells = cells;
    }
    HIPCHK(ctx, hipMemsetAsync(t->idx_id.p, 0xFF, cells * 8, st));
    HIPCHK(ctx, hipMemsetAsync(t->idx_slot.p, 0xFF, cells * 4, st));
    hipLaunchKernelGGL(meta_index_build_kernel, dim3(cdiv(slots, 256)), dim3(256), 0, st, (const uint64_t*)t->ids.as<uint64_t>(), slots,
                       t->idx_id.as<uint64_t>(), t->idx_slot.as<uint32_t>(), (uint32_t)(cells - 1));
    HIPCHK(ctx, hipGetLastError());
    t->idx_dirty = false;
  }
  const MetaCol& c = t->cols[column];
  hipLaunchKernelGGL(meta_keys_of_ids_kernel, dim3((uint32_t)cdiv(n, 256)), dim3(256), 0, st, ids_dev, n,
                     (const uint64_t*)t->idx_id.as<uint64_t>(), (const uint32_t*)t->idx_slot.as<uint32_t>(),
                     (uint32_t)(t->idx_cells ? t->idx_cells - 1 : 0), slots, (const uint8_t*)t->pres.as<uint8_t>(),
                     (const uint8_t*)c.tag.as<uint8_t>(), (const uint64_t*)c.val.as<uint64_t>(), out_tag_dev, out_key_dev);
  HIPCHK(ctx, hipGetLastError());
  return FVDB_OK;
}

// The context whose stream carries the lookup above: a caller that selects on another stream waits for this one first.
fvdb_ctx* fvdb_group_keys_ctx(fvdb_meta* t) { return t ? t->ctx : nullptr; }

}  // extern "C"
