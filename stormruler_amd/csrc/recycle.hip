// storm_hip_recycle: the initial guess of a solve projected onto the solutions of earlier solves with the same operator
// (Fischer 1998; the recipe: include/storm_hip.h).  This unit holds the object, the two ways through the recipe -- the
// fused kernels' launchers k_recycle_* (blas1.hip, beside the multi-dot / multi-axpy family they extend) and the
// statement path out of library launchers -- and the entry points.  Which access-mode instance a kernel runs is chosen
// inside the launchers, not here.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "common.hpp"

constexpr int kRecycleMax = 16;

struct storm_hip_recycle {
  storm_hip_ctx *ctx = nullptr;
  int64_t n_owned = 0, n_halo = 0;
  int capacity = 0, kind = 0, count = 0;
  bool coef_valid = false;  // a guess has stored c since the last update
  int64_t updates = 0, restarts = 0, device_bytes = 0;
  storm_hip_vec *uv[2][kRecycleMax] = {};  // the pairs
  double *u[kRecycleMax] = {}, *v[kRecycleMax] = {};  // ... their rows
  // the device scalars: g[16] c[16] e[16] beta[16] nu0 nu
  double *S = nullptr;
  double *g() const { return S; }
  double *c() const { return S + kRecycleMax; }
  double *e() const { return S + 2 * kRecycleMax; }
  double *beta() const { return S + 3 * kRecycleMax; }
  double *nu0() const { return S + 4 * kRecycleMax; }
  double *nu() const { return S + 4 * kRecycleMax + 1; }
};

namespace storm {

static int recycle_check_vec(const storm_hip_recycle *h, const storm_hip_vec *v, const char *who, const char *name) {
  STORM_REQUIRE(v->ctx == h->ctx, "%s: %s belongs to another context", who, name);
  STORM_REQUIRE(v->n_owned == h->n_owned, "%s: %s has %lld owned rows, the object %lld", who, name, (long long)v->n_owned,
                (long long)h->n_owned);
  return STORM_HIP_OK;
}

// <a, bs[j]>, j < k, into out: launches of at most kRecycleChunk sums, each finished inside its kernel
static int recycle_dots(storm_hip_ctx *c, const double *a, const double *const *bs, int k, int64_t n, double *out, int *launches) {
  for (int j0 = 0; j0 < k; j0 += kRecycleChunk) {
    const int kb = (k - j0) < kRecycleChunk ? (k - j0) : kRecycleChunk;
    STORM_TRY(k_multi_dot(c, a, bs + j0, kb, n, out + j0, nullptr));
    ++*launches;
  }
  return STORM_HIP_OK;
}

static int recycle_guess_run(storm_hip_recycle *h, const double *b, double *x) {
  storm_hip_ctx *c = h->ctx;
  const int64_t n = h->n_owned;
  const int k = h->count;
  const bool fused = c->opt_recycle_fused != 0;
  int launches = 0;
  if (n > 0) {
    if (k == 0) {
      STORM_TRY(k_fill(c, x, n, 0.0));
      ++launches;
    } else {
      const double *const *t = h->kind ? h->v : h->u;
      STORM_TRY(recycle_dots(c, b, t, k, n, h->e(), &launches));
      if (fused) {
        STORM_TRY(k_recycle_guess(c, n, x, h->u, k, h->g(), h->e(), h->c(), &launches));
      } else {
        STORM_TRY(k_recycle_scalar(c, 0, k, h->g(), h->e(), h->c(), nullptr, nullptr, 0, 0, &launches));
        STORM_TRY(k_fill(c, x, n, 0.0));
        STORM_TRY(k_multi_axpy(c, x, h->c(), 1.0, h->u, k, n, nullptr));
        launches += 1 + (k + kRecycleChunk - 1) / kRecycleChunk;
      }
    }
  }
  (fused ? c->n_recycle_fused_launches : c->n_recycle_statement_launches) += launches;
  h->coef_valid = k > 0 && n > 0;
  ++c->n_recycle_guesses;
  return STORM_HIP_OK;
}

static int recycle_update_run(storm_hip_recycle *h, const double *x, const double *ax) {
  storm_hip_ctx *c = h->ctx;
  const int64_t n = h->n_owned;
  const bool fused = c->opt_recycle_fused != 0, restart = h->count == h->capacity;
  const int kind = h->kind, s = restart ? 0 : h->count;
  int launches = 0;
  if (n > 0 && s == 0) {
    // (an empty object's first pair is the restart's: d = x, ad = ax, nu = nu0; every g_j above is zero already)
    if (fused) {
      STORM_TRY(k_recycle_restart(c, n, x, ax, h->u[0], h->v[0], kind, h->nu0(), h->nu(), h->g(), h->capacity, &launches));
    } else {
      STORM_TRY(k_copy(c, h->u[0], x, n, nullptr));
      STORM_TRY(k_copy(c, h->v[0], ax, n, nullptr));
      launches += 2;
      const double *w = kind ? h->v[0] : h->u[0];
      STORM_TRY(recycle_dots(c, h->v[0], &w, 1, n, h->nu(), &launches));
      STORM_TRY(k_recycle_scalar(c, 2, 0, h->g(), nullptr, nullptr, h->nu(), h->nu(), 0, h->capacity, &launches));
    }
  } else if (n > 0) {
    const double *coef = h->coef_valid ? h->c() : nullptr;
    if (fused) {
      STORM_TRY(k_recycle_defect(c, n, x, ax, h->u, h->v, s, coef, kind, h->e(), h->nu0(), &launches));
      STORM_TRY(k_recycle_orth(c, n, h->u, h->v, s, h->g(), h->e(), kind, h->nu0(), h->nu(), h->g(), &launches));
    } else {
      const int chunks = (s + kRecycleChunk - 1) / kRecycleChunk;
      STORM_TRY(k_copy(c, h->u[s], x, n, nullptr));
      STORM_TRY(k_copy(c, h->v[s], ax, n, nullptr));
      launches += 2;
      if (coef) {
        STORM_TRY(k_multi_axpy(c, h->u[s], coef, -1.0, h->u, s, n, nullptr));
        STORM_TRY(k_multi_axpy(c, h->v[s], coef, -1.0, h->v, s, n, nullptr));
        launches += 2 * chunks;
      }
      STORM_TRY(recycle_dots(c, h->v[s], kind ? h->v : h->u, s, n, h->e(), &launches));
      const double *w = kind ? h->v[s] : h->u[s];
      STORM_TRY(recycle_dots(c, h->v[s], &w, 1, n, h->nu0(), &launches));
      STORM_TRY(k_recycle_scalar(c, 0, s, h->g(), h->e(), h->beta(), nullptr, nullptr, 0, 0, &launches));
      STORM_TRY(k_multi_axpy(c, h->u[s], h->beta(), -1.0, h->u, s, n, nullptr));
      STORM_TRY(k_multi_axpy(c, h->v[s], h->beta(), -1.0, h->v, s, n, nullptr));
      launches += 2 * chunks;
      STORM_TRY(recycle_dots(c, h->v[s], &w, 1, n, h->nu(), &launches));
      STORM_TRY(k_recycle_scalar(c, 1, 0, h->g(), nullptr, nullptr, h->nu(), h->nu0(), s, 0, &launches));
    }
  }
  (fused ? c->n_recycle_fused_launches : c->n_recycle_statement_launches) += launches;
  h->count = s + 1;
  h->coef_valid = false;
  ++h->updates, ++c->n_recycle_updates;
  if (restart) ++h->restarts, ++c->n_recycle_restarts;
  return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" {

int storm_hip_recycle_create(storm_hip_ctx *ctx, int64_t n_owned, int64_t n_halo, int capacity, int kind, storm_hip_recycle **out) {
  STORM_REQUIRE(ctx && out, "recycle_create: null argument");
  *out = nullptr;
  STORM_REQUIRE(capacity >= 1 && capacity <= kRecycleMax, "recycle_create: capacity %d (1 .. %d)", capacity, kRecycleMax);
  STORM_REQUIRE(kind == STORM_HIP_RECYCLE_ENERGY || kind == STORM_HIP_RECYCLE_RESIDUAL, "recycle_create: kind %d (0: energy, 1: residual)", kind);
  STORM_REQUIRE(n_owned >= 0 && n_halo >= 0, "recycle_create: %lld owned rows, %lld halo rows", (long long)n_owned, (long long)n_halo);
  if (ctx->comm != nullptr)
    STORM_FAIL(STORM_HIP_E_UNSUPPORTED, "recycle_create: the sums of a recycler are local; a context with a communicator is not supported");
  STORM_TRY(lazy_sync(ctx));
  HIP_TRY(hipSetDevice(ctx->device));
  storm_hip_recycle *h = new storm_hip_recycle();
  h->ctx = ctx, h->n_owned = n_owned, h->n_halo = n_halo, h->capacity = capacity, h->kind = kind;
  int st = STORM_HIP_OK;
  const size_t scalar_bytes = sizeof(double) * (4 * kRecycleMax + 2);
  if (hipMalloc((void **)&h->S, scalar_bytes) != hipSuccess) {
    set_error("recycle_create: no device memory for the scalars");
    st = STORM_HIP_E_ALLOC;
  }
  if (st == STORM_HIP_OK && hipMemsetAsync(h->S, 0, scalar_bytes, ctx->stream) != hipSuccess) {
    set_error("recycle_create: hipMemsetAsync failed");
    st = STORM_HIP_E_HIP;
  }
  h->device_bytes = (int64_t)scalar_bytes;
  for (int j = 0; j < capacity && st == STORM_HIP_OK; ++j)
    for (int w = 0; w < 2 && st == STORM_HIP_OK; ++w) {
      st = storm_hip_vec_create(ctx, n_owned, n_halo, &h->uv[w][j]);
      if (st == STORM_HIP_OK) {
        (w ? h->v : h->u)[j] = h->uv[w][j]->d;
        h->device_bytes += (int64_t)h->uv[w][j]->bytes;
      }
    }
  if (st != STORM_HIP_OK) {
    (void)storm_hip_recycle_destroy(h);
    return st;
  }
  *out = h;
  return STORM_HIP_OK;
}

int storm_hip_recycle_destroy(storm_hip_recycle *h) {
  if (!h) return STORM_HIP_OK;
  (void)lazy_sync(h->ctx);
  for (int j = 0; j < kRecycleMax; ++j)
    for (int w = 0; w < 2; ++w)
      if (h->uv[w][j]) (void)storm_hip_vec_destroy(h->uv[w][j]);
  if (h->S) {
    (void)hipStreamSynchronize(h->ctx->stream);  // (a kernel may still be reading the scalars)
    (void)hipFree(h->S);
  }
  delete h;
  return STORM_HIP_OK;
}

int storm_hip_recycle_guess(storm_hip_recycle *h, const storm_hip_vec *b, storm_hip_vec *x) {
  STORM_REQUIRE(h && b && x, "recycle_guess: null argument");
  STORM_TRY(recycle_check_vec(h, b, "recycle_guess", "b"));
  STORM_TRY(recycle_check_vec(h, x, "recycle_guess", "x"));
  STORM_REQUIRE(x != b && x->d != b->d, "recycle_guess: x must not alias b");
  STORM_TRY(lazy_sync(h->ctx));
  HIP_TRY(hipSetDevice(h->ctx->device));
  return recycle_guess_run(h, b->d, x->d);
}

int storm_hip_recycle_update(storm_hip_recycle *h, const storm_hip_vec *x, const storm_hip_vec *ax) {
  STORM_REQUIRE(h && x && ax, "recycle_update: null argument");
  STORM_TRY(recycle_check_vec(h, x, "recycle_update", "x"));
  STORM_TRY(recycle_check_vec(h, ax, "recycle_update", "ax"));
  STORM_REQUIRE(x != ax && x->d != ax->d, "recycle_update: x must not alias ax");
  STORM_TRY(lazy_sync(h->ctx));
  HIP_TRY(hipSetDevice(h->ctx->device));
  return recycle_update_run(h, x->d, ax->d);
}

int storm_hip_recycle_reset(storm_hip_recycle *h) {
  STORM_REQUIRE(h, "recycle_reset: null argument");
  STORM_TRY(lazy_sync(h->ctx));
  HIP_TRY(hipSetDevice(h->ctx->device));
  HIP_TRY(hipMemsetAsync(h->g(), 0, sizeof(double) * kRecycleMax, h->ctx->stream));
  h->count = 0;
  h->coef_valid = false;
  return STORM_HIP_OK;
}

int storm_hip_recycle_get(const storm_hip_recycle *h, const char *key, double *value) {
  STORM_REQUIRE(h && key && value, "recycle_get: null argument");
  STORM_TRY(lazy_sync(h->ctx));
  if (!strcmp(key, "capacity")) *value = (double)h->capacity;
  else if (!strcmp(key, "count")) *value = (double)h->count;
  else if (!strcmp(key, "kind")) *value = (double)h->kind;
  else if (!strcmp(key, "updates")) *value = (double)h->updates;
  else if (!strcmp(key, "restarts")) *value = (double)h->restarts;
  else if (!strcmp(key, "device_bytes")) *value = (double)h->device_bytes;
  else if (!strncmp(key, "weight_", 7) || !strncmp(key, "coef_", 5)) {
    const bool weight = key[0] == 'w';
    const char *digits = key + (weight ? 7 : 5);
    char *end = nullptr;
    const long j = strtol(digits, &end, 10);
    STORM_REQUIRE(end != digits && *end == '\0' && j >= 0 && j < h->capacity, "recycle_get: '%s': no such slot (capacity %d)", key,
                  h->capacity);
    if (!weight && !h->coef_valid) {
      *value = 0.0;
      return STORM_HIP_OK;
    }
    HIP_TRY(hipSetDevice(h->ctx->device));
    HIP_TRY(hipStreamSynchronize(h->ctx->stream));
    HIP_TRY(hipMemcpy(value, (weight ? h->g() : h->c()) + j, sizeof(double), hipMemcpyDeviceToHost));
    if (!weight && j >= h->count) *value = 0.0;
  }
  else STORM_FAIL(STORM_HIP_E_INVALID, "recycle_get: unknown key '%s'", key);
  return STORM_HIP_OK;
}

int storm_hip_recycle_get_slot(const storm_hip_recycle *h, int j, storm_hip_vec *u, storm_hip_vec *v, double *g) {
  STORM_REQUIRE(h, "recycle_get_slot: null argument");
  STORM_REQUIRE(j >= 0 && j < h->count, "recycle_get_slot: slot %d of %d", j, h->count);
  if (u) STORM_TRY(recycle_check_vec(h, u, "recycle_get_slot", "u"));
  if (v) STORM_TRY(recycle_check_vec(h, v, "recycle_get_slot", "v"));
  STORM_TRY(lazy_sync(h->ctx));
  HIP_TRY(hipSetDevice(h->ctx->device));
  if (u) STORM_TRY(k_copy(h->ctx, u->d, h->u[j], h->n_owned, nullptr));
  if (v) STORM_TRY(k_copy(h->ctx, v->d, h->v[j], h->n_owned, nullptr));
  if (g) {
    HIP_TRY(hipStreamSynchronize(h->ctx->stream));
    HIP_TRY(hipMemcpy(g, h->g() + j, sizeof(double), hipMemcpyDeviceToHost));
  }
  return STORM_HIP_OK;
}

int storm_hip_recycle_set_slot(storm_hip_recycle *h, int j, const storm_hip_vec *u, const storm_hip_vec *v, double g) {
  STORM_REQUIRE(h && u && v, "recycle_set_slot: null argument");
  STORM_REQUIRE(j >= 0 && j <= h->count && j < h->capacity, "recycle_set_slot: slot %d (count %d, capacity %d)", j, h->count,
                h->capacity);
  STORM_TRY(recycle_check_vec(h, u, "recycle_set_slot", "u"));
  STORM_TRY(recycle_check_vec(h, v, "recycle_set_slot", "v"));
  STORM_TRY(lazy_sync(h->ctx));
  HIP_TRY(hipSetDevice(h->ctx->device));
  STORM_TRY(k_copy(h->ctx, h->u[j], u->d, h->n_owned, nullptr));
  STORM_TRY(k_copy(h->ctx, h->v[j], v->d, h->n_owned, nullptr));
  HIP_TRY(hipStreamSynchronize(h->ctx->stream));
  HIP_TRY(hipMemcpy(h->g() + j, &g, sizeof(double), hipMemcpyHostToDevice));
  if (j == h->count) ++h->count;
  h->coef_valid = false;
  return STORM_HIP_OK;
}

}  // extern "C"
