// srhip_lossx_run.inc — one run of a loss expression's register program over R rows per lane, included as
// text (not called) by lossx_kernel (srhip_lossx.hip) and rowsets_lossx_kernel (srhip_rowsets_lossx.hip), so
// both evaluate a row's loss with the same operator bodies in the same order.
// The including scope provides: T, R (rows per lane), O = FOps<T>, LX_PROG (the LossxProgram, in the kernel
// arguments: its instructions are read with scalar loads), vp[R], vy[R], vw[R] (prediction, target, weight).
// It declares the value slots s0 .. s7; slot 0 holds the rows' losses after the run.
// BODY with SLOT naming the value slot of wave-uniform index IDX.  The slots are eight separate arrays, not
// one two-dimensional array: over one array the optimiser folds the switch back into a runtime index, which
// sends the slots to scratch memory.
#define LX_WITH_SLOT(IDX, SLOT, BODY)                \
  switch (IDX) {                                     \
    case 0: { T(&SLOT)[R] = s0; BODY } break;        \
    case 1: { T(&SLOT)[R] = s1; BODY } break;        \
    case 2: { T(&SLOT)[R] = s2; BODY } break;        \
    case 3: { T(&SLOT)[R] = s3; BODY } break;        \
    case 4: { T(&SLOT)[R] = s4; BODY } break;        \
    case 5: { T(&SLOT)[R] = s5; BODY } break;        \
    case 6: { T(&SLOT)[R] = s6; BODY } break;        \
    default: { T(&SLOT)[R] = s7; BODY } break;       \
  }
        T s0[R], s1[R], s2[R], s3[R], s4[R], s5[R], s6[R], s7[R];
#pragma unroll
        for (int j = 0; j < R; ++j) s0[j] = s1[j] = s2[j] = s3[j] = s4[j] = s5[j] = s6[j] = s7[j] = T(0);
        for (int32_t pc = 0; pc < LX_PROG.n; ++pc) {
          const LossxIns I = LX_PROG.ins[pc];
          const uint32_t op = I.op;
          T a[R], b[R], v[R];
          if (op < LX_LOAD_PRED) {
            LX_WITH_SLOT(I.a, sl, {
              _Pragma("unroll") for (int j = 0; j < R; ++j) a[j] = sl[j];
            })
            if (op < SRHIP_OP_NEG) {
              LX_WITH_SLOT(I.b, sl, {
                _Pragma("unroll") for (int j = 0; j < R; ++j) b[j] = sl[j];
              })
            } else {
#pragma unroll
              for (int j = 0; j < R; ++j) b[j] = T(0);
            }
          } else {
#pragma unroll
            for (int j = 0; j < R; ++j) a[j] = b[j] = T(0);
          }
          switch (op) {
            case LX_LOAD_PRED:
#pragma unroll
              for (int j = 0; j < R; ++j) v[j] = vp[j];
              break;
            case LX_LOAD_Y:
#pragma unroll
              for (int j = 0; j < R; ++j) v[j] = vy[j];
              break;
            case LX_LOAD_W:
#pragma unroll
              for (int j = 0; j < R; ++j) v[j] = vw[j];
              break;
            case LX_LOAD_CONST: {
              const T c = imm_value<T>(I.imm);
#pragma unroll
              for (int j = 0; j < R; ++j) v[j] = c;
              break;
            }
#define X_(NAME, FN)                                        \
  case SRHIP_OP_##NAME:                                     \
    _Pragma("unroll") for (int j = 0; j < R; ++j) v[j] = O::FN(a[j], b[j]); \
    break;
              SRHIP_SPEC_BINOPS(X_)
              SRHIP_HEAVY_BINOPS(X_)
#undef X_
#define X_(NAME, FN)                                  \
  case SRHIP_OP_##NAME:                               \
    _Pragma("unroll") for (int j = 0; j < R; ++j) v[j] = O::FN(a[j]); \
    break;
              SRHIP_UNOPS(X_)
#undef X_
            default:
#pragma unroll
              for (int j = 0; j < R; ++j) v[j] = FP<T>::nan();
              break;
          }
          LX_WITH_SLOT(I.dst, sl, {
            _Pragma("unroll") for (int j = 0; j < R; ++j) sl[j] = v[j];
          })
        }
#undef LX_WITH_SLOT
