// srhip_grad_lossx_stage.inc — the loss stage of the constant-gradient kernels under a loss expression,
// included as text (not called) by grad_lossx_kernel (srhip_grad_lossx.hip) and grad_rowsets_lossx_kernel
// (srhip_grad_rowsets_lossx.hip) between parts 1 and 3 of srhip_grad_tile.inc, so both run the same
// arithmetic in the same order and neither kernel's code generation depends on the other.
// The including scope provides: T, KT, K, R, DL (KT > 0), A[R] and S[K][R] of part 1, lane, tb, nrel, yat(rr),
// W, row_base, lx_w (the program reads the weight and there is one), lx_n (instructions), GLX_PROG (the
// LossxProgram, in the kernel arguments), lacc, gacc.
// BODY with (SV, SD) naming the value and tangent slot of wave-uniform index IDX.  Separate arrays behind a
// switch, as in lossx_kernel: one runtime-indexed array sends the slots to scratch memory.
#define GLX_WITH_SLOT(IDX, SV, SD, BODY)                                 \
  switch (IDX) {                                                         \
    case 0: { T(&SV)[R] = v0; T(&SD)[R] = d0; (void)SD; BODY } break;    \
    case 1: { T(&SV)[R] = v1; T(&SD)[R] = d1; (void)SD; BODY } break;    \
    case 2: { T(&SV)[R] = v2; T(&SD)[R] = d2; (void)SD; BODY } break;    \
    case 3: { T(&SV)[R] = v3; T(&SD)[R] = d3; (void)SD; BODY } break;    \
    case 4: { T(&SV)[R] = v4; T(&SD)[R] = d4; (void)SD; BODY } break;    \
    case 5: { T(&SV)[R] = v5; T(&SD)[R] = d5; (void)SD; BODY } break;    \
    case 6: { T(&SV)[R] = v6; T(&SD)[R] = d6; (void)SD; BODY } break;    \
    default: { T(&SV)[R] = v7; T(&SD)[R] = d7; (void)SD; BODY } break;   \
  }
      // ---- the loss stage: the tree's stack S is dead from here; the program's slots take its registers
      {
        // (the stack's last values would otherwise stay live through the stage and round the tile loop: an
        // unwritten slot of the next tile's S is "any value", which the optimiser takes to be this tile's)
        UNR for (int k = 0; k < K; ++k)
          UNR for (int r = 0; r < R; ++r) {
            S[k][r].v = T(0);
            UNR for (int j = 0; j < KT; ++j) S[k][r].d[j] = T(0);
          }
        T vy[R], vw[R];
        UNR for (int r = 0; r < R; ++r) {
          const int rr = tb + 64 * r + lane;
          const bool in = rr < nrel;
          vy[r] = in ? yat(rr) : T(0);
          vw[r] = (in && lx_w) ? W[row_base + rr] : T(0);
        }
        T v0[R], v1[R], v2[R], v3[R], v4[R], v5[R], v6[R], v7[R];
        T d0[R], d1[R], d2[R], d3[R], d4[R], d5[R], d6[R], d7[R];
        UNR for (int r = 0; r < R; ++r) {
          v0[r] = v1[r] = v2[r] = v3[r] = v4[r] = v5[r] = v6[r] = v7[r] = T(0);
          d0[r] = d1[r] = d2[r] = d3[r] = d4[r] = d5[r] = d6[r] = d7[r] = T(0);
        }
        for (int pc = 0; pc < lx_n; ++pc) {
          const LossxIns I = GLX_PROG.ins[pc];
          const uint32_t op = I.op;
          T a[R], b[R], da[R], db[R], v[R], dv[R];
          UNR for (int r = 0; r < R; ++r) a[r] = b[r] = da[r] = db[r] = dv[r] = T(0);
          if (op < LX_LOAD_PRED) {
            GLX_WITH_SLOT(I.a, sv, sd, {
              UNR for (int r = 0; r < R; ++r) { a[r] = sv[r]; if constexpr (DL) da[r] = sd[r]; }
            })
            if (op < SRHIP_OP_NEG) {
              GLX_WITH_SLOT(I.b, sv, sd, {
                UNR for (int r = 0; r < R; ++r) { b[r] = sv[r]; if constexpr (DL) db[r] = sd[r]; }
              })
            }
          }
          switch (op) {
            case LX_LOAD_PRED:
              UNR for (int r = 0; r < R; ++r) { v[r] = A[r].v; dv[r] = T(1); }
              break;
            case LX_LOAD_Y:
              UNR for (int r = 0; r < R; ++r) v[r] = vy[r];
              break;
            case LX_LOAD_W:
              UNR for (int r = 0; r < R; ++r) v[r] = vw[r];
              break;
            case LX_LOAD_CONST: {
              const T c = imm_bits<T>(I.imm);
              UNR for (int r = 0; r < R; ++r) v[r] = c;
              break;
            }
#define X_(NAME, FN)                                                                   \
  case SRHIP_OP_##NAME:                                                                \
    UNR for (int r = 0; r < R; ++r) {                                                  \
      T f, fa, fb;                                                                     \
      dual_spec<T, SB_##NAME>(a[r], b[r], f, fa, fb);                                  \
      v[r] = f;                                                                        \
      if constexpr (DL) dv[r] = fa * da[r] + fb * db[r];                               \
    }                                                                                  \
    break;
              SRHIP_SPEC_BINOPS(X_)
#undef X_
#define X_(NAME, FN)                                                                   \
  case SRHIP_OP_##NAME:                                                                \
    UNR for (int r = 0; r < R; ++r) {                                                  \
      const typename V4<T>::type h = dual_heavy<T, HB_##NAME, DL>(a[r], b[r]);         \
      v[r] = h[0];                                                                     \
      if constexpr (DL) dv[r] = h[1] * da[r] + h[2] * db[r];                           \
    }                                                                                  \
    break;
              SRHIP_HEAVY_BINOPS(X_)
#undef X_
#define X_(NAME, FN)                                                                   \
  case SRHIP_OP_##NAME:                                                                \
    UNR for (int r = 0; r < R; ++r) {                                                  \
      T f, df;                                                                         \
      dual_un<T, UN_##NAME, DL>(a[r], f, df);                                          \
      v[r] = f;                                                                        \
      if constexpr (DL) dv[r] = df * da[r];                                            \
    }                                                                                  \
    break;
              SRHIP_UNOPS(X_)
#undef X_
            default:
              UNR for (int r = 0; r < R; ++r) { v[r] = FP<T>::nan(); dv[r] = FP<T>::nan(); }
              break;
          }
          GLX_WITH_SLOT(I.dst, sv, sd, {
            UNR for (int r = 0; r < R; ++r) { sv[r] = v[r]; if constexpr (DL) sd[r] = dv[r]; }
          })
        }
        // part 2's fold: ascending row order within the lane, the product in T
        UNR for (int r = 0; r < R; ++r) {
          const int rr = tb + 64 * r + lane;
          if (rr < nrel) {
            const T l = v0[r], dl = d0[r];
            (void)dl;
            lacc += (double)l;
            UNR for (int j = 0; j < KT; ++j) gacc[j] += (double)(dl * A[r].d[j]);
          }
        }
      }
#undef GLX_WITH_SLOT
