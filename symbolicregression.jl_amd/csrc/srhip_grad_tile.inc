// srhip_grad_tile.inc — the dual-number interpreter's tile body, included as text (not called) by grad_kernel
// (srhip_grad.hip), grad_rowsets_kernel (srhip_grad_rowsets.hip) and the two kernels with a loss expression's
// stage in place of part 2 (srhip_grad_lossx.hip, srhip_grad_rowsets_lossx.hip), so all run the same arithmetic
// in the same order and no kernel's code generation depends on another.  SRHIP_GRAD_PART selects the section:
//   1  one tile of one chunk: the bytecode loop over A[R] / S[K][R] (values, tangents, check fold M)
//   2  the tile's rows folded into lacc / gacc[] in ascending row order (rows >= nrel masked)
//   3  the six xor levels that turn the lanes' sums into the (chunk, row block) record
// The including scope provides: T, KT, K, GM, R, p (nfeat, ld, gd_nd, loss_kind, weighted), lane, tb, nrel, c0,
// code, pc0, max_steps, p0, Xg, W, row_base, xat(f, rr), yat(rr), M, lacc, gacc.
#if SRHIP_GRAD_PART == 1
      Dual<T, KT> A[R], S[K][R];
      UNR for (int r = 0; r < R; ++r) set_feat<GMODE_LOSS>(A[r], T(0), -1);
      GIns* prog = code + pc0;
      Ins nxt = prog[0];
      for (int step = 0; step < max_steps; ++step) {
        const Ins ins = nxt;
        nxt = prog[step + 1];
        if (ins.h == H_END) break;
        const int opnd = (int)(ins.a & 0xffff);
        const T imm = imm_bits<T>(ins.imm);
#define RR(...) UNR for (int r = 0; r < R; ++r) { const int rr = tb + 64 * r + lane; (void)rr; __VA_ARGS__ }
        switch (ins.h) {
          case H_LOADF:
            RR(set_feat<GM>(A[r], xat(opnd, rr), opnd - c0);)
            if (opnd >= p.nfeat) {
              // a derived column: the operator's output (its check fold), and its tangents f'(x) * 0
              // (+-0, or NaN where f' is not finite) from the tangent-zero column
              RR(chk_fold(M, A[r].v);)
              if constexpr (KT > 0) {
                RR(const T z = Xg[(int64_t)(opnd + p.gd_nd) * p.ld + row_base + rr];
                   UNR for (int j = 0; j < KT; ++j) A[r].d[j] = z;)
              }
            }
            break;
          case H_LOADC: RR(set_const<GM>(A[r], imm, opnd - c0);) break;
#define GK_CASES(BASE, ...)                                                                        \
  case BASE + 0: if constexpr (0 < K) { constexpr int k = 0; __VA_ARGS__ } break;                \
  case BASE + 1: if constexpr (1 < K) { constexpr int k = 1; __VA_ARGS__ } break;                \
  case BASE + 2: if constexpr (2 < K) { constexpr int k = 2; __VA_ARGS__ } break;                \
  case BASE + 3: if constexpr (3 < K) { constexpr int k = 3; __VA_ARGS__ } break;                \
  case BASE + 4: if constexpr (4 < K) { constexpr int k = 4; __VA_ARGS__ } break;                \
  case BASE + 5: if constexpr (5 < K) { constexpr int k = 5; __VA_ARGS__ } break;                \
  case BASE + 6: if constexpr (6 < K) { constexpr int k = 6; __VA_ARGS__ } break;                \
  case BASE + 7: if constexpr (7 < K) { constexpr int k = 7; __VA_ARGS__ } break;
          GK_CASES(H_PUSH0, { RR(S[k][r] = A[r];) })
#if SRHIP_GRAD_SUPER_LEVEL >= 1
          // superinstructions (round 6): a push fused with the plain feature / constant load after it
          GK_CASES(H_PUSHLF0, { RR(S[k][r] = A[r]; set_feat<GM>(A[r], xat(opnd, rr), opnd - c0);) })
          GK_CASES(H_PUSHLC0, { RR(S[k][r] = A[r]; set_const<GM>(A[r], imm, opnd - c0);) })
#endif
          GK_CASES(H_SLOADF0, { RR(set_feat<GM>(S[k][r], xat(opnd, rr), opnd - c0);) })
          GK_CASES(H_SLOADC0, { RR(set_const<GM>(S[k][r], imm, opnd - c0);) })
// (AC / CA / SA / AS forms with UN_UNIFORM_FLAG in the operand field: two constant subtrees, one
// value per lane -- row 0 evaluated, copied to the others with their check folds)
#define GK_UNI_ROWS()                                                                              \
  UNR for (int r = 1; r < R; ++r) A[r] = A[0];                                                     \
  UNR for (int r = 0; r < R; ++r) chk_fold(M, A[r].v);
#if SRHIP_GRAD_SUPER_LEVEL >= 2
#define GK_LEAFLEAF(NAME)                                                                          \
  /* leaf-leaf forms (round 6): X[a] op X[imm], X[a] op c, c op X[a] -- c's index in the upper half */ \
  case h_spec(SB_##NAME, SPEC_FF): {                                                               \
    const int f2 = (int)(ins.imm & 0xffff);                                                        \
    RR(Dual<T, KT> o; set_feat<GM>(A[r], xat(opnd, rr), opnd - c0); set_feat<GM>(o, xat(f2, rr), f2 - c0); \
       T f, fl, fr; dual_spec<T, SB_##NAME>(A[r].v, o.v, f, fl, fr); combine(A[r], A[r], o, f, fl, fr); \
       chk_fold(M, A[r].v);) break; }                                                              \
  case h_spec(SB_##NAME, SPEC_FC): {                                                               \
    const int ci = (int)(ins.a >> 16) - c0;                                                        \
    RR(Dual<T, KT> o; set_feat<GM>(A[r], xat(opnd, rr), opnd - c0); set_const<GM>(o, imm, ci);     \
       T f, fl, fr; dual_spec<T, SB_##NAME>(A[r].v, o.v, f, fl, fr); combine(A[r], A[r], o, f, fl, fr); \
       chk_fold(M, A[r].v);) break; }                                                              \
  case h_spec(SB_##NAME, SPEC_CF): {                                                               \
    const int ci = (int)(ins.a >> 16) - c0;                                                        \
    RR(Dual<T, KT> o; set_feat<GM>(A[r], xat(opnd, rr), opnd - c0); set_const<GM>(o, imm, ci);     \
       T f, fl, fr; dual_spec<T, SB_##NAME>(o.v, A[r].v, f, fl, fr); combine(A[r], o, A[r], f, fl, fr); \
       chk_fold(M, A[r].v);) break; }
#else
#define GK_LEAFLEAF(NAME)
#endif
#define GK_SPEC(NAME, FN)                                                                          \
  GK_LEAFLEAF(NAME)                                                                                \
  case h_spec(SB_##NAME, SPEC_AF): {                                                               \
    RR(Dual<T, KT> o; set_feat<GM>(o, xat(opnd, rr), opnd - c0);                                   \
       T f, fl, fr; dual_spec<T, SB_##NAME>(A[r].v, o.v, f, fl, fr); combine(A[r], A[r], o, f, fl, fr); \
       chk_fold(M, A[r].v);) break; }                                                              \
  case h_spec(SB_##NAME, SPEC_FA): {                                                               \
    RR(Dual<T, KT> o; set_feat<GM>(o, xat(opnd, rr), opnd - c0);                                   \
       T f, fl, fr; dual_spec<T, SB_##NAME>(o.v, A[r].v, f, fl, fr); combine(A[r], o, A[r], f, fl, fr); \
       chk_fold(M, A[r].v);) break; }                                                              \
  case h_spec(SB_##NAME, SPEC_AC): {                                                               \
    const int ci = (opnd & ~(int)UN_UNIFORM_FLAG) - c0;                                            \
    if (R > 1 && (ins.a & UN_UNIFORM_FLAG)) {                                                      \
      Dual<T, KT> o; set_const<GM>(o, imm, ci);                                                    \
      T f, fl, fr; dual_spec<T, SB_##NAME>(A[0].v, o.v, f, fl, fr); combine(A[0], A[0], o, f, fl, fr); \
      GK_UNI_ROWS() break;                                                                         \
    }                                                                                              \
    RR(Dual<T, KT> o; set_const<GM>(o, imm, ci);                                                   \
       T f, fl, fr; dual_spec<T, SB_##NAME>(A[r].v, o.v, f, fl, fr); combine(A[r], A[r], o, f, fl, fr); \
       chk_fold(M, A[r].v);) break; }                                                              \
  case h_spec(SB_##NAME, SPEC_CA): {                                                               \
    const int ci = (opnd & ~(int)UN_UNIFORM_FLAG) - c0;                                            \
    if (R > 1 && (ins.a & UN_UNIFORM_FLAG)) {                                                      \
      Dual<T, KT> o; set_const<GM>(o, imm, ci);                                                    \
      T f, fl, fr; dual_spec<T, SB_##NAME>(o.v, A[0].v, f, fl, fr); combine(A[0], o, A[0], f, fl, fr); \
      GK_UNI_ROWS() break;                                                                         \
    }                                                                                              \
    RR(Dual<T, KT> o; set_const<GM>(o, imm, ci);                                                   \
       T f, fl, fr; dual_spec<T, SB_##NAME>(o.v, A[r].v, f, fl, fr); combine(A[r], o, A[r], f, fl, fr); \
       chk_fold(M, A[r].v);) break; }                                                              \
  GK_CASES(h_spec(SB_##NAME, SPEC_SA0), {                                                          \
    if (R > 1 && (ins.a & UN_UNIFORM_FLAG)) {                                                      \
      T f, fl, fr; dual_spec<T, SB_##NAME>(S[k][0].v, A[0].v, f, fl, fr);                          \
      combine(A[0], S[k][0], A[0], f, fl, fr); GK_UNI_ROWS() break;                                \
    }                                                                                              \
    RR(T f, fl, fr; dual_spec<T, SB_##NAME>(S[k][r].v, A[r].v, f, fl, fr);                         \
       combine(A[r], S[k][r], A[r], f, fl, fr); chk_fold(M, A[r].v);) })                           \
  GK_CASES(h_spec(SB_##NAME, SPEC_AS0), {                                                          \
    if (R > 1 && (ins.a & UN_UNIFORM_FLAG)) {                                                      \
      T f, fl, fr; dual_spec<T, SB_##NAME>(A[0].v, S[k][0].v, f, fl, fr);                          \
      combine(A[0], A[0], S[k][0], f, fl, fr); GK_UNI_ROWS() break;                                \
    }                                                                                              \
    RR(T f, fl, fr; dual_spec<T, SB_##NAME>(A[r].v, S[k][r].v, f, fl, fr);                         \
       combine(A[r], A[r], S[k][r], f, fl, fr); chk_fold(M, A[r].v);) })
          SRHIP_SPEC_BINOPS(GK_SPEC)
#undef GK_SPEC
#undef GK_LEAFLEAF
#define GK_HEAVY(NAME, FN)                                                                         \
  GK_CASES(h_heavy(HB_##NAME, HEAVY_SA0), {                                                        \
    RR(const typename V4<T>::type q = dual_heavy<T, HB_##NAME, (KT > 0)>(S[k][r].v, A[r].v);                 \
       combine(A[r], S[k][r], A[r], q[0], q[1], q[2]); chk_fold(M, A[r].v);) })                    \
  GK_CASES(h_heavy(HB_##NAME, HEAVY_AS0), {                                                        \
    RR(const typename V4<T>::type q = dual_heavy<T, HB_##NAME, (KT > 0)>(A[r].v, S[k][r].v);                 \
       combine(A[r], A[r], S[k][r], q[0], q[1], q[2]); chk_fold(M, A[r].v);) })
          SRHIP_HEAVY_BINOPS(GK_HEAVY)
#undef GK_HEAVY
#define GK_UN(NAME, FN)                                                                            \
  case h_un(UN_##NAME): {                                                                          \
    if (R > 1 && (ins.a & UN_UNIFORM_FLAG)) {  /* a constant subtree's rows: one evaluation */     \
      T f, df;                                                                                     \
      dual_un<T, UN_##NAME, (KT > 0)>(A[0].v, f, df);                                              \
      A[0].v = f;                                                                                  \
      UNR for (int j = 0; j < KT; ++j) A[0].d[j] = df * A[0].d[j];                                 \
      UNR for (int r = 0; r < R; ++r) { A[r] = A[0]; chk_fold(M, A[r].v); }                        \
      break;                                                                                       \
    }                                                                                              \
    if constexpr (KT == 0 && !dun_inline<UN_##NAME>()) {                                           \
      typename VR<T, R>::type xv;                                                                  \
      if constexpr (R == 1) xv = A[0].v;                                                           \
      else { UNR for (int r = 0; r < R; ++r) xv[r] = A[r].v; }                                     \
      xv = dual_un_heavy_rows<T, UN_##NAME, R>(xv);                                                \
      if constexpr (R == 1) { A[0].v = xv; chk_fold(M, A[0].v); }                                  \
      else { UNR for (int r = 0; r < R; ++r) { A[r].v = xv[r]; chk_fold(M, A[r].v); } }            \
      break;                                                                                       \
    }                                                                                              \
    RR(T f, df; dual_un<T, UN_##NAME, (KT > 0)>(A[r].v, f, df);                                              \
       A[r].v = f;                                                                                 \
       UNR for (int j = 0; j < KT; ++j) A[r].d[j] = df * A[r].d[j];                                \
       chk_fold(M, A[r].v);) break; }
          SRHIP_UNOPS(GK_UN)
#undef GK_UN
#undef GK_CASES
          default: break;
        }
#undef RR
      }
#elif SRHIP_GRAD_PART == 2
      UNR for (int r = 0; r < R; ++r) {
        const int rr = tb + 64 * r + lane;
        if (rr < nrel) {
          const T d = A[r].v - yat(rr);
          T l, dl;
          if (p.loss_kind == SRHIP_LOSS_L2) {
            l = d * d;
            dl = T(2) * d;
          } else {
            const typename V2<T>::type q = loss_dloss_generic<T>(p.loss_kind, A[r].v, yat(rr), p0);
            l = q[0];
            dl = q[1];
          }
          if (p.weighted) {
            const T w = W[row_base + rr];
            l = w * l;
            dl = w * dl;
          }
          lacc += (double)l;
          UNR for (int j = 0; j < KT; ++j) gacc[j] += (double)(dl * A[r].d[j]);
        }
      }
#elif SRHIP_GRAD_PART == 3
    auto level = [&](auto oc) {
      constexpr int O = decltype(oc)::value;
      lacc += xor_lane<O>(lacc, lane);
      UNR for (int j = 0; j < KT; ++j) gacc[j] += xor_lane<O>(gacc[j], lane);
      if constexpr (sizeof(T) == 4) M = __builtin_elementwise_maximum(M, xor_lane<O>(M, lane));
      else M += xor_lane<O>(M, lane);
    };
    level(std::integral_constant<int, 32>());
    level(std::integral_constant<int, 16>());
    level(std::integral_constant<int, 8>());
    level(std::integral_constant<int, 4>());
    level(std::integral_constant<int, 2>());
    level(std::integral_constant<int, 1>());
#endif
