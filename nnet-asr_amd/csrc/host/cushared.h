// cushared.h -- <sharedlinearity> and <blockarray>, the layers of the convolutive-bottleneck /
// universal-context networks.
//
// CuSharedLinearity : src/CuTNetLib/cuSharedLinearity.h:15-85, .cc:10-176 (CPU twin: src/TNetLib/SharedLinearity.cc)
// CuBlockArray      : src/CuTNetLib/cuBlockArray.h:18-83, .cc:10-135      (CPU twin: src/TNetLib/BlockArray.cc)
//
// One weight matrix [in/N x out/N] applied to the N column blocks of the input: each of Propagate,
// Backpropagate and Update is ONE instance-batched kernel call (tnet_shared_fwd / _bwd / _update,
// gemm_shared.hip) where the reference makes N OffsetGemm calls.  A block array runs parallel sub-networks on
// column stripes, forward only, as in the reference.
#pragma once

#include <vector>

#include "cucomponent.h"

namespace TNet {

class CuNetwork;

class CuSharedLinearity : public CuUpdatableComponent {
 public:
  CuSharedLinearity(size_t nInputs, size_t nOutputs, CuComponent* pPred)
      : CuUpdatableComponent(nInputs, nOutputs, pPred), mNInstances(0) {}

  ComponentType GetType() const override { return SHARED_LINEARITY; }
  bool IsRowWise() const override { return true; }
  const char* GetName() const override { return "<sharedlinearity>"; }

  void PropagateFnc(const CuMatrix<BaseFloat>& X, CuMatrix<BaseFloat>& Y) override;
  void BackpropagateFnc(const CuMatrix<BaseFloat>& X, CuMatrix<BaseFloat>& Y) override;
  /// cuSharedLinearity.cc:65-94 in one fused call
  void Update() override;
  /// Update() split around a data-parallel gradient exchange: the gradient over all instances and the bias gradient
  /// (tnet_shared_grad) into buffers of the parameters' layout ([in x stride] and the bias, allocated on the first
  /// data-parallel step), then the flat SGD apply over the element ranges the exchange hands this rank
  /// (all-reduce and sharded apply alike), with UpdateConstants(global rows): the instance factor stays
  void ComputeGradient() override;
  void ApplyGradient(size_t frames, void* stream = nullptr, const GradExchange* ex = nullptr) override;
  std::vector<CuParamBlock> GradientBlocks() override;

  void ReadFromStream(std::istream& rIn) override;
  void WriteToStream(std::ostream& rOut) override;

  /// SGD constants of CuSharedLinearity::Update (cuSharedLinearity.cc:67-75, 89-93) for `rows` frames; unlike
  /// CuBiasedLinearity's, the weight decay carries no rows factor
  void UpdateConstants(size_t rows, float* scale, float* l2) const;

  int NInstances() const { return mNInstances; }
  CuMatrix<BaseFloat>& Linearity() { return mLinearity; }
  CuVector<BaseFloat>& Bias() { return mBias; }

 protected:
  CuMatrix<BaseFloat> mLinearity;            ///< [nIn/N x nOut/N] (file stores the transpose)
  CuVector<BaseFloat> mBias;                 ///< [nOut/N]
  CuMatrix<BaseFloat> mLinearityCorrection;  ///< momentum buffer
  CuVector<BaseFloat> mBiasCorrection;       ///< momentum buffer
  CuMatrix<BaseFloat> mGradW;                ///< data-parallel gradient buffers (lazily allocated, zeroed)
  CuVector<BaseFloat> mGradB;
  int mNInstances;
};

class CuBlockArray : public CuUpdatableComponent {
 public:
  CuBlockArray(size_t nInputs, size_t nOutputs, CuComponent* pPred)
      : CuUpdatableComponent(nInputs, nOutputs, pPred), mNBlocks(0) {}
  ~CuBlockArray();

  ComponentType GetType() const override { return BLOCK_ARRAY; }
  const char* GetName() const override { return "<blockarray>"; }

  void PropagateFnc(const CuMatrix<BaseFloat>& X, CuMatrix<BaseFloat>& Y) override;
  void BackpropagateFnc(const CuMatrix<BaseFloat>& X, CuMatrix<BaseFloat>& Y) override;  ///< "Unimplemented"
  void Update() override;                                                                 ///< "Unimplemented"

  void ReadFromStream(std::istream& rIn) override;
  void WriteToStream(std::ostream& rOut) override;

  int NBlocks() const { return mNBlocks; }

 protected:
  std::vector<CuNetwork*> mBlocks;  ///< owned
  // per block: its column stripe of the input and its output (kept between bunches: no allocation in a step)
  std::vector<CuMatrix<BaseFloat>*> mStripeIn, mStripeOut;
  int mNBlocks;
};

}  // namespace TNet
