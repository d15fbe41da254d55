// cudiscrete.h -- <discretelinearity>, the block-diagonal trainable layer of band-split / hierarchical
// bottleneck networks.
//
// CuDiscreteLinearity : src/CuTNetLib/cuDiscreteLinearity.h, .cc:9-156 (no CPU twin in src/TNetLib)
//
// Block k has its own weight matrix [in_k x out_k] between its column stripe of the input and its stripe of the
// output; one bias covers the whole output.  Each of Propagate, Backpropagate and Update is ONE grouped kernel
// call over all blocks (tnet_discrete_fwd / _bwd / _update, gemm_discrete.hip) where the reference loops over
// OffsetGemm.  The blocks' matrices live in one packed device buffer whose layout the plan fixes at load time.
#pragma once

#include <vector>

#include "cucomponent.h"

namespace TNet {

class CuDiscreteLinearity : public CuUpdatableComponent {
 public:
  CuDiscreteLinearity(size_t nInputs, size_t nOutputs, CuComponent* pPred)
      : CuUpdatableComponent(nInputs, nOutputs, pPred), mNBlocks(0), mpPlan(nullptr) {}
  ~CuDiscreteLinearity();
  CuDiscreteLinearity(const CuDiscreteLinearity&) = delete;  // owns the plan
  CuDiscreteLinearity& operator=(const CuDiscreteLinearity&) = delete;

  ComponentType GetType() const override { return DISCRETE_LINEARITY; }
  bool IsRowWise() const override { return true; }
  const char* GetName() const override { return "<discretelinearity>"; }

  void PropagateFnc(const CuMatrix<BaseFloat>& X, CuMatrix<BaseFloat>& Y) override;
  void BackpropagateFnc(const CuMatrix<BaseFloat>& X, CuMatrix<BaseFloat>& Y) override;
  /// cuDiscreteLinearity.cc:45-78 in one fused call
  void Update() override;
  /// Update() split around a data-parallel gradient exchange: every block's gradient and the bias gradient
  /// (tnet_discrete_grad) into one buffer of the plan's packed layout and one of the bias's (allocated on the
  /// first data-parallel step), then the flat SGD apply over the element ranges the exchange hands this rank
  /// (all-reduce and sharded apply alike), with UpdateConstants(global rows)
  void ComputeGradient() override;
  void ApplyGradient(size_t frames, void* stream = nullptr, const GradExchange* ex = nullptr) override;
  std::vector<CuParamBlock> GradientBlocks() override;

  void ReadFromStream(std::istream& rIn) override;
  void WriteToStream(std::ostream& rOut) override;

  /// SGD constants of CuDiscreteLinearity::Update (cuDiscreteLinearity.cc:50-55, 69-71) for `rows` frames: no
  /// block-count factor (unlike CuSharedLinearity's instance factor) and no rows factor in the weight decay
  /// (unlike CuBiasedLinearity's)
  void UpdateConstants(size_t rows, float* scale, float* l2) const;

  int NBlocks() const { return mNBlocks; }
  size_t BlockInputs(int k) const { return (size_t)mIn[k]; }
  size_t BlockOutputs(int k) const { return (size_t)mOut[k]; }
  /// block k's matrix, host row-major [in_k x out_k] with row stride ld
  void GetBlock(int k, BaseFloat* W, size_t ld) const;
  void SetBlock(int k, const BaseFloat* W, size_t ld);
  CuVector<BaseFloat>& Bias() { return mBias; }

 protected:
  CuVector<BaseFloat> mLinearity;            ///< every W_k [in_k x out_k], packed (file stores the transposes)
  CuVector<BaseFloat> mBias;                 ///< [nOut]
  CuVector<BaseFloat> mLinearityCorrection;  ///< momentum buffer, packed like mLinearity
  CuVector<BaseFloat> mBiasCorrection;       ///< momentum buffer
  CuVector<BaseFloat> mGradW, mGradB;        ///< data-parallel gradient buffers (lazily allocated, zeroed)
  std::vector<int> mIn, mOut;               ///< block dimensions
  int mNBlocks;
  double mMacsPerRow = 0.0;                  ///< sum in_k * out_k (profiling only)
  TnetDiscretePlan* mpPlan;                  ///< packed layout + device tables of the grouped kernels (owned)
};

}  // namespace TNet
