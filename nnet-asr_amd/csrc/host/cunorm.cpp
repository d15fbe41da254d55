// cunorm.cpp -- CuNormAccumulator (cunorm.h): the TNormCu loop over the device front end and tnet_col_moments.
#include "cunorm.h"

#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>

#include "htkio.h"

namespace TNet {

CuNormAccumulator::CuNormAccumulator(CuNetwork* transform, size_t dim, size_t start_ext, size_t end_ext,
                                     bool count_ext_frames)
    : mTransform(transform), mDim(transform && transform->Layers() ? transform->GetNOutputs() : dim),
      mStartExt(start_ext), mEndExt(end_ext), mCountExt(count_ext_frames) {
  if (mDim == 0 || mDim > (size_t)1 << 24) Error("CuNormAccumulator: the dimension must be positive");
  CuDevice& dev = CuDevice::Instantiate();
  mAccBytes = (size_t)tnet_col_moments_words((int)mDim) * sizeof(double);
  mAcc = (double*)dev.Alloc(mAccBytes);
  TNET_HIP_CALL(hipMemsetAsync(mAcc, 0, mAccBytes, dev.Stream()));
  for (int k = 0; k < 2; k++) TNET_HIP_CALL(hipEventCreateWithFlags(&mCopied[k], hipEventDisableTiming));
}

CuNormAccumulator::~CuNormAccumulator() {
  // the accumulator and the staging buffers may still be read by enqueued work
  (void)hipStreamSynchronize(CuDevice::Instantiate().Stream());
  CuDevice::Instantiate().Free(mAcc, mAccBytes);
  for (int k = 0; k < 2; k++) {
    if (mPinned[k]) (void)hipHostFree(mPinned[k]);
    if (mCopied[k]) (void)hipEventDestroy(mCopied[k]);
  }
}

void CuNormAccumulator::AddUtterance(const float* feats, size_t rows_ext, size_t cols, size_t ld,
                                     const std::string& name) {
  if (mCollected) Error("CuNormAccumulator::AddUtterance: the statistics have already been fetched");
  if (rows_ext < mStartExt + mEndExt + 1) {
    std::ostringstream os;
    os << "CuNormAccumulator::AddUtterance: " << rows_ext << " rows cannot carry " << mStartExt << " + " << mEndExt
       << " context rows";
    Error(os.str());
  }
  if (!feats || cols == 0 || ld < cols) Error("CuNormAccumulator::AddUtterance: bad feature matrix");
  if (mNames.size() >= (size_t)0x7fffffff) Error("CuNormAccumulator::AddUtterance: too many utterances");
  const bool through = mTransform && mTransform->Layers() > 0;
  if (through ? cols != mTransform->GetNInputs() : cols != mDim) {
    std::ostringstream os;
    os << "CuNormAccumulator::AddUtterance: feature dim " << cols << " != "
       << (through ? "transform input dim " : "accumulator dim ") << (through ? mTransform->GetNInputs() : mDim);
    Error(os.str());
  }
  const size_t rows = rows_ext - mStartExt - mEndExt;
  const int tag = (int)mNames.size();
  hipStream_t st = CuDevice::Instantiate().Stream();

  // host rows -> pinned staging buffer tag % 2 (waiting only for the copy of utterance tag - 2) -> device
  const int k = tag & 1;
  if (mInFlight[k]) {
    TNET_HIP_CALL(hipEventSynchronize(mCopied[k]));
    mInFlight[k] = false;
  }
  const size_t need = rows_ext * cols;
  if (need > mPinnedFloats[k]) {
    if (mPinned[k]) TNET_HIP_CALL(hipHostFree(mPinned[k]));
    mPinned[k] = nullptr;
    mPinnedFloats[k] = 0;
    const size_t cap = need + need / 2;
    TNET_HIP_CALL(hipHostMalloc((void**)&mPinned[k], cap * sizeof(float), hipHostMallocDefault));
    mPinnedFloats[k] = cap;
  }
  for (size_t r = 0; r < rows_ext; r++) std::memcpy(mPinned[k] + r * cols, feats + r * ld, cols * sizeof(float));
  mRaw.CopyFromHost(mPinned[k], rows_ext, cols, cols, /*sync=*/false);
  TNET_HIP_CALL(hipEventRecord(mCopied[k], st));
  mInFlight[k] = true;

  const CuMatrix<BaseFloat>* out = &mRaw;
  if (through) {
    mTransform->Propagate(mRaw, mOut);
    out = &mOut;
  }
  // the trimmed rows as a view of the output: no CopyRows, no CopyTo
  TnetMatrixDim d = out->Dim();
  d.rows = (int)rows;
  TNET_SAFE_CALL(tnet_col_moments(out->pCURowData(mStartExt), d, mAcc, tag, st));
  mNames.push_back(name);
  mSummed += rows;
  mFrames += mCountExt ? rows_ext : rows;  // TNormCu.cc:286 counts feats_host.Rows()
}

long CuNormAccumulator::AddReader(tnetio::FeatureReader& reader, size_t reader_start_ext, size_t reader_end_ext,
                                  long max_utts) {
  if (reader_start_ext != mStartExt || reader_end_ext != mEndExt) {
    std::ostringstream os;
    os << "CuNormAccumulator::AddReader: the reader carries " << reader_start_ext << "/" << reader_end_ext
       << " context rows, the accumulator expects " << mStartExt << "/" << mEndExt;
    Error(os.str());
  }
  const unsigned long before = mSummed;
  for (long n = 0; max_utts < 0 || n < max_utts; n++) {
    const tnetio::Utterance* u = reader.Next();
    if (!u) break;
    AddUtterance(u->feats.data(), (size_t)u->rows, (size_t)u->cols, (size_t)u->cols, u->logical);
  }
  return (long)(mSummed - before);
}

void CuNormAccumulator::Collect() {
  if (mCollected) return;
  mFirst.assign(mDim, 0.0);
  mSecond.assign(mDim, 0.0);
  TNET_SAFE_CALL(tnet_col_moments_fetch(mAcc, (int)mDim, mFirst.data(), mSecond.data(), &mBadTag,
                                        CuDevice::Instantiate().Stream()));
  mInFlight[0] = mInFlight[1] = false;  // the fetch drained the stream
  mCollected = true;
}

void CuNormAccumulator::CheckBad() const {
  if (mBadTag < 0) return;
  std::ostringstream os;
  os << "nan/inf in accumulators\nutterance index:" << mBadTag;
  if ((size_t)mBadTag < mNames.size() && !mNames[(size_t)mBadTag].empty()) os << "\nutterance:" << mNames[(size_t)mBadTag];
  os << "\n";
  Error(os.str());
}

const std::vector<double>& CuNormAccumulator::First() {
  Collect();
  return mFirst;
}
const std::vector<double>& CuNormAccumulator::Second() {
  Collect();
  return mSecond;
}

void CuNormAccumulator::Merge(GradExchange& ex) {
  if (mFinished) Error("CuNormAccumulator::Merge: only before Finish");
  Collect();
  CheckBad();  // before the collective: a rank that throws later would leave the others waiting
  std::vector<double> v(2 * mDim + 1);
  std::memcpy(v.data(), mFirst.data(), mDim * sizeof(double));
  std::memcpy(v.data() + mDim, mSecond.data(), mDim * sizeof(double));
  v[2 * mDim] = (double)mFrames;
  ex.AllReduceHost(v.data(), (int)v.size());
  std::memcpy(mFirst.data(), v.data(), mDim * sizeof(double));
  std::memcpy(mSecond.data(), v.data() + mDim, mDim * sizeof(double));
  mFrames = (unsigned long)v[2 * mDim];
}

void CuNormAccumulator::Finish() {
  if (mFinished) return;
  Collect();
  CheckBad();
  mBias.resize(mDim);
  mWindow.resize(mDim);
  // TNormCu.cc:298-317: Scale(1.0 / framesN), then the same operations element by element
  const double scale = 1.0 / (double)mFrames;
  for (size_t i = 0; i < mDim; i++) {
    const double mean = mFirst[i] * scale;
    double variance = mSecond[i] * scale;
    variance -= mean * mean;
    mBias[i] = mean * -1.0;
    mWindow[i] = 1.0 / std::sqrt(variance);
  }
  mFinished = true;
}

const std::vector<double>& CuNormAccumulator::Bias() const {
  if (!mFinished) Error("CuNormAccumulator: Finish() first");
  return mBias;
}
const std::vector<double>& CuNormAccumulator::Window() const {
  if (!mFinished) Error("CuNormAccumulator: Finish() first");
  return mWindow;
}

size_t CuNormAccumulator::BadWindowEntries() const {
  size_t n = 0;
  for (double w : Window()) n += std::isfinite(w) ? 0 : 1;
  return n;
}

// KaldiLib's operator<<(ostream&, const Vector<double>&) (Vector.tcc:550-571): "v D  " and every element followed by a
// blank, at the stream's own (default: 6 significant digits) precision -- the double itself, not a float of it
static void PutVector(std::ostream& os, const std::vector<double>& v) {
  os << "v " << v.size() << "  ";
  for (double x : v) os << x << ' ';
}

void CuNormAccumulator::WriteToStream(std::ostream& os) const {
  const std::vector<double>&bias = Bias(), &window = Window();
  os << "<bias> " << mDim << " " << mDim << "\n";
  PutVector(os, bias);
  os << "\n\n"
     << "<window> " << mDim << " " << mDim << "\n";
  PutVector(os, window);
  os << "\n\n";
}

void CuNormAccumulator::Write(const char* path) const {
  std::ofstream os(path);
  if (!os.good()) Error(std::string("Cannot open file for writing: ") + path);
  WriteToStream(os);
  os.close();
  if (os.fail()) Error(std::string("Failed to write: ") + path);
}

std::string CuNormAccumulator::Report() const {
  const std::vector<double>&bias = Bias(), &window = Window();
  // Vector::Max / Min (Vector.tcc): start from the first element, keep the larger / smaller
  double max_bias = bias[0], max_window = window[0], min_window = window[0];
  for (size_t i = 1; i < mDim; i++) {
    if (bias[i] > max_bias) max_bias = bias[i];
    if (window[i] > max_window) max_window = window[i];
    if (window[i] < min_window) min_window = window[i];
  }
  std::ostringstream os;
  os << "frames: " << mFrames << ", max_bias: " << max_bias << ", max_window: " << max_window
     << ", min_window: " << min_window << "\n";
  return os.str();
}

}  // namespace TNet
