// curve_bls377.hip — instantiates the prover for BLS12-377 (/root/reference/zokrates_field/src/bls12_377.rs).
#include "core.cuh"
namespace zk {
const CurveOps* curve_ops_bls377() {
    static const CurveOps ops = make_curve_ops<CurveBls377>();
    return &ops;
}
}  // namespace zk
