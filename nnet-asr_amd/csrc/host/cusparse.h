// cusparse.h -- <sparselinearity>, the masked, L1-regularised affine layer (what TNetCu's --L1 option acts on).
//
// CuSparseLinearity : src/CuTNetLib/cuSparseLinearity.h, .cc:11-186 (no CPU twin in src/TNetLib)
//
// A dense W [n_in x n_out] with a 0/1 sparsity mask of the same shape, an L1 soft threshold and a running sum of
// the momentum buffer (`accu`) that UpdateMask uses to wake weights up again.  Propagate and Backpropagate are the
// library's dense affine GEMMs (W holds exact zeros under the mask); Update is ONE fused call
// (tnet_sparse_update, gemm_sparse.hip) where the reference runs a GEMM and five element-wise passes over W.  The
// mask lives on the device as a bit matrix (32 columns per word).
#pragma once

#include "cucomponent.h"

namespace TNet {

class CuSparseLinearity : public CuUpdatableComponent {
 public:
  CuSparseLinearity(size_t nInputs, size_t nOutputs, CuComponent* pPred)
      : CuUpdatableComponent(nInputs, nOutputs, pPred) {}

  ComponentType GetType() const override { return SPARSE_LINEARITY; }
  bool IsRowWise() const override { return true; }
  const char* GetName() const override { return "<sparselinearity>"; }

  void PropagateFnc(const CuMatrix<BaseFloat>& X, CuMatrix<BaseFloat>& Y) override;
  void BackpropagateFnc(const CuMatrix<BaseFloat>& X, CuMatrix<BaseFloat>& Y) override;
  /// cuSparseLinearity.cc:28-63 in one fused call
  void Update() override;
  /// Update() split around a data-parallel gradient exchange.  The gradient X^T E and colsum(E) comes from
  /// tnet_sparse_grad, on Update()'s tile core and in its summation order (the dense layer's tnet_affine_grad sums
  /// in another order, and accu, a running sum that cancels, then misses the one-rank tolerance against the fused
  /// step), into buffers of W's pitched layout and the bias's, allocated on the first data-parallel step.  The
  /// apply runs Update()'s per-element arithmetic
  /// on the reduced gradient (tnet_sparse_apply per element range, the bias through tnet_sgd_update_multi) with
  /// UpdateConstants(global rows), and the frame count grows by the global rows -- also on a rank that joined the
  /// step without a bunch.
  /// NOT under the sharded apply (TNET_DP_SHARD=1): there a rank holds the reduced gradient of its shard only, so
  /// `accu`, which UpdateMask reads over the whole matrix, would differ from rank to rank and the masks would
  /// drift apart.  CuNetwork refuses such a step before its first collective -- whatever the rank count: a
  /// one-rank run with the variable exported is refused too.
  void ComputeGradient() override;
  void ApplyGradient(size_t frames, void* stream = nullptr, const GradExchange* ex = nullptr) override;
  std::vector<CuParamBlock> GradientBlocks() override;
  /// cuSparseLinearity.cc:66-97 on the device: cut active weights below the sparsify threshold, wake inactive ones
  /// whose |accu| / nframes exceeds the unsparsify threshold.  Runs at the start of every WriteToStream.
  void UpdateMask();

  /// the mask matrix and the accu matrix in the file are optional; accu is read and dropped (.cc:100-160)
  void ReadFromStream(std::istream& rIn) override;
  /// UpdateMask(), then W^T, b, mask^T, accu^T (.cc:163-186)
  void WriteToStream(std::ostream& rOut) override;

  /// SGD constants of CuSparseLinearity::Update (.cc:32-37, 50-58) for `rows` frames
  void UpdateConstants(size_t rows, float* scale, float* l1c, float* l2) const;

  void L1(BaseFloat l1) { mL1Const = l1; }
  BaseFloat L1() const { return mL1Const; }
  void SparsifyWeightThreshold(BaseFloat t) { mSparsifyWeightThreshold = t; }
  BaseFloat SparsifyWeightThreshold() const { return mSparsifyWeightThreshold; }
  void UnsparsifyAccu(BaseFloat t) { mUnsparsifyAccu = t; }
  BaseFloat UnsparsifyAccu() const { return mUnsparsifyAccu; }
  long NFrames() const { return mNFrames; }

  CuMatrix<BaseFloat>& Linearity() { return mLinearity; }
  CuVector<BaseFloat>& Bias() { return mBias; }
  CuMatrix<BaseFloat>& Accu() { return mLinearityCorrectionAccu; }
  /// the mask as 0/1 floats, host row-major [n_in x n_out] with row stride ld
  void GetMask(BaseFloat* mask, size_t ld) const;
  /// nonzero -> 1; W is not touched
  void SetMask(const BaseFloat* mask, size_t ld);

 protected:
  size_t MaskStride() const { return (mLinearity.Cols() + 31) / 32; }

  CuMatrix<BaseFloat> mLinearity;                ///< [nIn x nOut] (file stores the transpose)
  CuVector<BaseFloat> mBias;                     ///< [nOut]
  CuVector<int> mSparsityMask;                   ///< bit matrix: nIn rows of ceil(nOut / 32) words
  CuMatrix<BaseFloat> mLinearityCorrection;      ///< momentum buffer
  CuVector<BaseFloat> mBiasCorrection;           ///< momentum buffer
  CuMatrix<BaseFloat> mLinearityCorrectionAccu;  ///< running sum of mLinearityCorrection
  CuMatrix<BaseFloat> mGradW;                    ///< data-parallel gradient buffers (lazily allocated, zeroed)
  CuVector<BaseFloat> mGradB;
  long mNFrames = 0;
  BaseFloat mL1Const = 0.0f;
  BaseFloat mSparsifyWeightThreshold = 1.0e-3f;
  BaseFloat mUnsparsifyAccu = 1e20f;
};

}  // namespace TNet
