// batch_driver.cpp -- TEST INFRASTRUCTURE: drives the batch entry points of the host runtime (pockit_amd/csrc/pk_batch.cpp) against
// the host-only HIP stand-in of this directory, built with -fsanitize=address,undefined (tests/test_cycle_batch_host_sanitized.py):
// one launch of pk_cycleb per batch with pk_cycle's grid and LDS, the record copy in front of every launch, the per-entry
// workspaces over changes of B and of the problem, the hand-off slots of every entry put back after error 97, the loop of single cycles for a model that needs the integrals first (checked
// against what the stand-in's "kernels" write for THAT entry), the refusals, tear-down without a live allocation.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "driver_common.h"
#include "../../pockit_amd/csrc/pk_runtime.h"      // (the context itself: the status words and the hand-off slots of a batch)

static std::vector<std::string> ops_since(size_t mark) {
  const auto& lg = fake_hip_log();
  return std::vector<std::string>(lg.begin() + (long)mark, lg.end());
}

int main() {
  FakeSizes S;
  S.n = 40; S.m = 30; S.nnz_J = 200; S.nnz_H = 150;
  fake_hip_set_sizes(S);
  OK(pk_create(&ctx, 0));
  pk_model_desc md{};
  md.n_phase = 1; md.n_I = 1; md.nred = 1; md.lds_g = md.lds_j = md.lds_h = md.lds_x = md.lds_e = md.lds_jc = 64;
  md.ne_j = md.ne_h = md.ne_a = 1; md.prepass_f = 1; md.tab_cap = 64;
  CHECK(pk_load_batch_model(ctx, image, sizeof image) == 2);      // no model yet
  OK(pk_load_model(ctx, image, sizeof image, &md));
  PkPhase ph{};
  PkTile tiles[2 * PK_WAVES_PER_BLOCK] = {};
  for (auto& t : tiles) t.K = 1;
  ph.tile_hi = 2 * PK_WAVES_PER_BLOCK;
  pk_problem_desc pd{};
  pd.n = S.n; pd.m = S.m; pd.n_phase = 1; pd.nnz_J = S.nnz_J; pd.nnz_H = S.nnz_H;
  pd.phases = &ph; pd.tiles = tiles; pd.n_tiles = 2 * PK_WAVES_PER_BLOCK;
  CHECK(pk_set_batch(ctx, 2) == 3);                                // no problem yet
  OK(pk_set_problem(ctx, &pd));

  const int B = 5;
  std::vector<double> X((size_t)B * (S.n + 3)), L((size_t)B * S.m), sig(B), f(B), grad((size_t)B * S.n), g((size_t)B * S.m),
      J((size_t)B * S.nnz_J), H((size_t)B * S.nnz_H, -7.25);
  for (size_t i = 0; i < X.size(); ++i) X[i] = 0.5 + 0.001 * (double)i;
  for (size_t i = 0; i < L.size(); ++i) L[i] = 1.0 - 0.002 * (double)i;
  for (int b = 0; b < B; ++b) sig[b] = 1.0 - 0.125 * b;
  const int64_t ldx = S.n + 3;
  auto eval = [&](int nb, const double* lam) {
    return pk_eval_cycle_batch_dev(ctx, nb, X.data(), ldx, lam, S.m, lam ? sig.data() : nullptr, f.data(), grad.data(), g.data(),
                                   J.data(), lam ? H.data() : nullptr, nullptr);
  };

  // ---- no batched object: the loop of single cycles (the stand-in's pk_cycle writes recomputable values)
  size_t mark = fake_hip_log().size(), launches = fake_hip_launches().size();
  OK(eval(3, L.data()));
  OK(pk_sync(ctx, nullptr));
  CHECK(fake_hip_launches().size() == launches + 3);
  const unsigned cycle_grid = fake_hip_launches().back().grid;
  const size_t cycle_lds = fake_hip_launches().back().lds_bytes;
  CHECK(fake_hip_launches().back().kernel == "pk_cycle");
  for (int b = 0; b < 3; ++b) {
    const double* x = X.data() + (size_t)b * ldx;
    CHECK(f[b] == fake_f(x, S.n));
    for (int64_t i = 0; i < S.n; ++i) CHECK(grad[(size_t)b * S.n + i] == fake_grad(x, S.n, i));
    for (int64_t j = 0; j < S.m; ++j) CHECK(g[(size_t)b * S.m + j] == fake_g(x, S.n, j));
    for (int64_t p = 0; p < S.nnz_J; ++p) CHECK(J[(size_t)b * S.nnz_J + p] == fake_jac(x, S.n, p, false));
    for (int64_t p = 0; p < S.nnz_H; ++p)
      CHECK(H[(size_t)b * S.nnz_H + p] == fake_hess(x, L.data() + (size_t)b * S.m, sig[b], S.n, S.m, p));
  }
  for (int64_t p = 0; p < S.nnz_H; ++p) CHECK(H[3 * (size_t)S.nnz_H + p] == -7.25);      // (entry 3 was not part of the batch)

  // ---- with the batched object: ONE launch per batch, the records in front of it
  OK(pk_load_batch_model(ctx, image, sizeof image));
  mark = fake_hip_log().size(); launches = fake_hip_launches().size();
  OK(eval(B, L.data()));
  {
    const auto ops = ops_since(mark);
    CHECK(ops.size() >= 2 && ops[ops.size() - 2] == "h2d" && ops.back() == "pk_cycleb");
    CHECK(fake_hip_launches().size() == launches + 1);
    const FakeLaunch& l = fake_hip_launches().back();
    CHECK(l.kernel == "pk_cycleb" && l.grid == cycle_grid && l.lds_bytes == cycle_lds && l.arg_bytes == 32);
  }
  mark = fake_hip_log().size();
  OK(eval(B, L.data()));                                            // the same batch again: the records go up with every launch
  CHECK((ops_since(mark) == std::vector<std::string>{"h2d", "pk_cycleb"}));
  for (int k = 0; k < 9; ++k) {                                     // batches back to back, nothing waited for by the caller
    sig[2] = 0.01 * k;
    OK(eval(k % B + 1, k % 2 ? L.data() : nullptr));
  }
  OK(pk_sync(ctx, nullptr));

  // ---- error 97 for a batch: a finalize workgroup of SOME entry gave up (the shared status word counts it), tile workgroups
  //      that published afterwards left their values in that entry's slots -- the check puts the slots of every entry back
  {
    const size_t slots = 2 * ctx->batch.n_partial * (size_t)ctx->batch.cap;
    CHECK(ctx->batch.cap == B && slots > 0);
    for (size_t i = 0; i < slots; ++i) CHECK(ctx->batch.d_cp[i] == (unsigned long long)PK_EMPTY);
    const size_t late = 2 * ctx->batch.n_partial * 3 + 1;           // (a slot of entry 3)
    ctx->batch.d_cp[late] = 0x3FF0000000000000ull;
    ctx->batch.d_cp[slots - 1] = 0x4000000000000000ull;
    unsigned long long* status = reinterpret_cast<unsigned long long*>(ctx->shim.res[0].h_out + 6);
    status[0] += 1;
    CHECK(pk_sync(ctx, nullptr) == 97);
    for (size_t i = 0; i < slots; ++i) CHECK(ctx->batch.d_cp[i] == (unsigned long long)PK_EMPTY);
    OK(pk_sync(ctx, nullptr));                                      // reported once
    OK(eval(B, L.data()));
    OK(pk_sync(ctx, nullptr));
  }
  OK(pk_set_batch(ctx, 2));                                         // a smaller batch keeps the workspaces
  OK(pk_set_batch(ctx, PK_MAX_BATCH));                              // the largest replaces them
  OK(eval(B, L.data()));
  OK(pk_sync(ctx, nullptr));

  // ---- refusals
  CHECK(pk_set_batch(ctx, 0) == 87 && pk_set_batch(ctx, PK_MAX_BATCH + 1) == 87);
  CHECK(eval(PK_MAX_BATCH + 1, L.data()) == 87 && eval(0, L.data()) == 87);
  CHECK(pk_eval_cycle_batch_dev(ctx, 2, X.data(), S.n - 1, L.data(), S.m, sig.data(), f.data(), grad.data(), g.data(), J.data(),
                                H.data(), nullptr) == 89);
  CHECK(pk_eval_cycle_batch_dev(ctx, 2, X.data(), ldx, L.data(), S.m, sig.data(), f.data(), grad.data(), g.data(), J.data(),
                                nullptr, nullptr) == 89);

  // ---- the two-launch cycle and a new problem: the loop again, the workspaces freed with the problem
  OK(pk_set_cycle_mode(ctx, 0));
  launches = fake_hip_launches().size();
  OK(eval(2, L.data()));
  OK(pk_sync(ctx, nullptr));
  CHECK(fake_hip_launches().size() == launches + 4 && fake_hip_launches().back().kernel == "pk_hess");
  OK(pk_set_cycle_mode(ctx, 1));
  OK(pk_set_problem(ctx, &pd));
  OK(eval(2, L.data()));
  OK(pk_sync(ctx, nullptr));
  CHECK(fake_hip_launches().back().kernel == "pk_cycleb");
  OK(pk_load_batch_model(ctx, nullptr, 0));                         // dropped: single cycles
  OK(eval(2, L.data()));
  OK(pk_sync(ctx, nullptr));
  CHECK(fake_hip_launches().back().kernel == "pk_cycle");
  OK(pk_load_batch_model(ctx, image, sizeof image));
  OK(eval(2, L.data()));
  pk_destroy(ctx);
  ctx = nullptr;
  CHECK(fake_hip_live_allocations() == 0);
  return checks_passed();
}
