// cunorm.h -- CuNormAccumulator: the TNormCu loop (src/TNormCu.cc:215-343) as a library object.
//
// TNormCu computes the global mean / variance normalisation that every recipe `cat`s onto its feature
// transform: per utterance it propagates the (frame-extended) features through the transform, trims the context
// rows, and adds every element and its square into two double vectors; at the end
//   mean = first / N,  var = second / N - mean^2,  <bias> = -mean,  <window> = 1 / sqrt(var)
// are written as a two-component .nnet text.  The reference copies every transformed utterance back and
// accumulates on one host thread; here the sums stay on the device (tnet_col_moments on a row-offset view of the
// transform's output -- no trimmed copy, no copy back), the uploads go through two pinned staging buffers, and
// the only device-to-host traffic is one fetch at the end.  Nothing synchronises per utterance except the
// reuse of a staging buffer two utterances later.
//
// The frame-count quirk.  TNormCu.cc:286 counts `feats_host.Rows()` -- the rows INCLUDING the STARTFRMEXT +
// ENDFRMEXT context frames -- while the sums cover only the trimmed rows.  With the recipes' +-25 frames on
// examples/01 that is N = 60,457 for 55,457 summed frames: the "mean" is 0.917 of the true mean and the
// variance is off accordingly.  Every existing transform was made this way, so count_ext_frames = true (the
// default) reproduces it; false divides by the rows that were summed.
//
// A zero or negative variance gives inf / nan in <window>, exactly as in the reference (no clamp);
// BadWindowEntries() counts them.  An utterance that makes an accumulator NaN / Inf (some transformed value or
// its fp32 square is not finite) is found at Finish / Merge from the device-side tag, and named in the
// reference's words ("nan/inf in accumulators").
#pragma once

#include <iostream>
#include <string>
#include <vector>

#include "cunetwork.h"
#include "gradexchange.h"

namespace tnetio {
class FeatureReader;
}

namespace TNet {

class CuNormAccumulator {
 public:
  /// transform: borrowed, may be nullptr (then `dim` is the feature dimension; with a transform `dim` is ignored
  /// and the dimension is the transform's output dimension)
  CuNormAccumulator(CuNetwork* transform, size_t dim, size_t start_ext, size_t end_ext, bool count_ext_frames = true);
  ~CuNormAccumulator();
  CuNormAccumulator(const CuNormAccumulator&) = delete;
  CuNormAccumulator& operator=(const CuNormAccumulator&) = delete;

  size_t Dim() const { return mDim; }
  /// One utterance as FeatureRepository delivers it: rows_ext rows including the start_ext / end_ext context
  /// rows (host memory, leading dimension ld).  `name`: its logical name for the error report (may be empty).
  void AddUtterance(const float* feats, size_t rows_ext, size_t cols, size_t ld, const std::string& name = "");
  /// Up to max_utts utterances (< 0: to the end of the list) from a reader whose frame extension is
  /// reader_start_ext / reader_end_ext (must be this accumulator's); returns the frames summed.
  long AddReader(tnetio::FeatureReader& reader, size_t reader_start_ext, size_t reader_end_ext, long max_utts);
  /// Data parallel: first, second and the frame count summed over the ranks (one all-reduce of 2 Dim + 1
  /// doubles); every rank then holds the corpus statistics.  A rank holding a bad utterance throws before the
  /// collective.  Only before Finish.
  void Merge(GradExchange& ex);
  /// mean / variance -> bias / window (TNormCu.cc:298-317), in double on the host
  void Finish();
  bool Finished() const { return mFinished; }

  /// the sums so far (one fetch from the device the first time; no utterance can be added afterwards)
  const std::vector<double>& First();
  const std::vector<double>& Second();
  unsigned long Frames() const { return mFrames; }        ///< N of the division (see the quirk above)
  unsigned long SummedFrames() const { return mSummed; }  ///< rows that entered the sums
  const std::vector<double>& Bias() const;
  const std::vector<double>& Window() const;
  size_t BadWindowEntries() const;  ///< inf / nan entries of <window> (zero or negative variance)

  void WriteToStream(std::ostream& os) const;  ///< TNormCu.cc:320-327
  void Write(const char* path) const;
  std::string Report() const;  ///< "frames: ... , max_bias: ... , max_window: ... , min_window: ...\n"

 private:
  void Collect();
  void CheckBad() const;

  CuNetwork* mTransform;
  size_t mDim, mStartExt, mEndExt;
  bool mCountExt;
  double* mAcc = nullptr;  // device accumulator of tnet_col_moments (belongs to the library stream)
  size_t mAccBytes = 0;
  // pinned upload staging: utterance k goes through buffer k % 2, reused once its copy has completed
  float* mPinned[2] = {nullptr, nullptr};
  size_t mPinnedFloats[2] = {0, 0};
  hipEvent_t mCopied[2] = {nullptr, nullptr};
  bool mInFlight[2] = {false, false};
  CuMatrix<BaseFloat> mRaw, mOut;
  std::vector<std::string> mNames;  // per utterance index (the tag)
  unsigned long mFrames = 0, mSummed = 0;
  bool mCollected = false, mFinished = false;
  int mBadTag = -1;
  std::vector<double> mFirst, mSecond, mBias, mWindow;
};

}  // namespace TNet
