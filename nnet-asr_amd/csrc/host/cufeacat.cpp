// cufeacat.cpp -- CuFeaCat (cufeacat.h): the TFeaCatCu loop over packed utterances and the emit kernels.
#include "cufeacat.h"

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <sstream>

#include "htkio.h"

namespace TNet {

CuFeaCat::CuFeaCat(CuNetwork* net, CuNetwork* transform, size_t start_ext, size_t end_ext, int mode, size_t pack_rows,
                   bool pack)
    : mNet(net), mTransform(transform && transform->Layers() ? transform : nullptr), mStartExt(start_ext),
      mEndExt(end_ext), mMode(mode), mPackRows(pack_rows ? pack_rows : kDefaultPackRows) {
  if (!net) Error("CuFeaCat: a network is required (an empty one copies the transform's output)");
  if (mode < 0 || mode > (TNET_FEACAT_GMMBYPASS | TNET_FEACAT_LOGPOSTERIOR)) Error("CuFeaCat: unknown mode bits");
  if (mPackRows > (size_t)1 << 24) Error("CuFeaCat: pack_rows too large");
  const int n = net->Layers();
  if (n && mTransform && mTransform->GetNOutputs() != net->GetNInputs()) {
    std::ostringstream os;
    os << "CuFeaCat: the feature transform's output dimension " << mTransform->GetNOutputs()
       << " differs from the network's input dimension " << net->GetNInputs();
    Error(os.str());
  }
  mPacked = pack;
  for (int i = 0; i < n; i++) mPacked = mPacked && net->Layer(i).IsRowWise();
  mSoftmaxTop = n > 0 && net->Layer(n - 1).GetType() == CuComponent::SOFTMAX;
  mC = n ? net->GetNOutputs() : mTransform ? mTransform->GetNOutputs() : 0;  // 0: the features' own dimension
  mNetIn = n ? net->GetNInputs() : mC;
  if (mC) CheckDims(mC);
  TNET_HIP_CALL(hipStreamCreateWithFlags(&mCopyStream, hipStreamNonBlocking));
  for (int k = 0; k < 2; k++) TNET_HIP_CALL(hipEventCreateWithFlags(&mCopied[k], hipEventDisableTiming));
  for (Slot& s : mSlot) {
    TNET_HIP_CALL(hipEventCreateWithFlags(&s.emitted, hipEventDisableTiming));
    TNET_HIP_CALL(hipEventCreateWithFlags(&s.drained, hipEventDisableTiming));
  }
}

CuFeaCat::~CuFeaCat() {
  StopWriters();
  // the buffers may still be read or written by enqueued work
  (void)hipStreamSynchronize(CuDevice::Instantiate().Stream());
  if (mCopyStream) (void)hipStreamSynchronize(mCopyStream);
  for (int k = 0; k < 2; k++) {
    if (mPinned[k]) (void)hipHostFree(mPinned[k]);
    if (mCopied[k]) (void)hipEventDestroy(mCopied[k]);
  }
  for (Result& r : mResults)  // a pass that was never finished
    if (r.fd >= 0) {
      close(r.fd);
      remove(r.path.c_str());
    }
  for (Slot& s : mSlot) {
    if (s.dense) CuDevice::Instantiate().Free(s.dense, s.cap * sizeof(uint32_t));
    if (s.pinned) (void)hipHostFree(s.pinned);
    if (s.emitted) (void)hipEventDestroy(s.emitted);
    if (s.drained) (void)hipEventDestroy(s.drained);
  }
  if (mCopyStream) (void)hipStreamDestroy(mCopyStream);
}

void CuFeaCat::CheckDims(size_t cols) {
  if (cols > 8191) {
    std::ostringstream os;
    os << "CuFeaCat: " << cols << " output columns do not fit the 16-bit sample size of an HTK header (at most 8191)";
    Error(os.str());
  }
}

void CuFeaCat::SetOutput(const char* dir, const char* ext, bool swap, int writer_threads) {
  if (mStarted) Error("CuFeaCat::SetOutput: only before the first utterance");
  if (writer_threads < 1 || writer_threads > 16) Error("CuFeaCat::SetOutput: 1 to 16 writer threads");
  mFile = true;
  mHasDir = dir != nullptr;
  mDir = dir ? dir : "";
  mExt = ext ? ext : "";
  mSwap = swap;
  mWriterThreads = writer_threads;
}

void CuFeaCat::SetSwap(bool swap) {
  if (mStarted) Error("CuFeaCat::SetSwap: only before the first utterance");
  mSwap = swap;
}

void CuFeaCat::Reserve(Slot& s, size_t words) {
  if (words <= s.cap) return;
  if (s.in_flight) Error("CuFeaCat: slot resized while in flight");
  CuDevice& dev = CuDevice::Instantiate();
  if (s.dense) {
    // the emit that wrote it and the copy that read it have completed (the slot was drained), but the allocator
    // hands the block to whatever asks next on the library stream: order it behind the copy stream anyway
    TNET_HIP_CALL(hipStreamSynchronize(mCopyStream));
    dev.Free(s.dense, s.cap * sizeof(uint32_t));
    s.dense = nullptr;
  }
  if (s.pinned) TNET_HIP_CALL(hipHostFree(s.pinned));
  s.pinned = nullptr;
  s.cap = 0;
  const size_t cap = mPacked ? words : words + words / 2;
  s.dense = (uint32_t*)dev.Alloc(cap * sizeof(uint32_t));
  TNET_HIP_CALL(hipHostMalloc((void**)&s.pinned, cap * sizeof(uint32_t), hipHostMallocDefault));
  s.cap = cap;
}

void CuFeaCat::AddUtterance(const float* feats, size_t rows_ext, size_t cols, size_t ld, const std::string& logical,
                            int sample_period) {
  if (mFinished) Error("CuFeaCat::AddUtterance: the pass has been finished");
  const std::string who = logical.empty() ? std::string("utterance ") + std::to_string(mUtts) : logical;
  if (rows_ext <= mStartExt + mEndExt) {
    std::ostringstream os;
    os << "CuFeaCat: " << who << ": " << rows_ext << " rows cannot carry " << mStartExt << " + " << mEndExt
       << " context rows";
    Error(os.str());
  }
  if (!feats || cols == 0 || ld < cols) Error("CuFeaCat: " + who + ": bad feature matrix");
  const size_t want = mTransform ? mTransform->GetNInputs() : mNetIn ? mNetIn : cols;
  if (cols != want) {
    std::ostringstream os;
    os << "CuFeaCat: " << who << ": feature dimension " << cols << " != "
       << (mTransform ? "the feature transform's" : "the network's") << " input dimension " << want;
    Error(os.str());
  }
  if (!mC) {  // neither a transform nor a network: the features themselves
    CheckDims(cols);
    mC = mNetIn = cols;
  }
  if (!mStarted) {
    mStarted = true;
    if (mFile)
      for (int t = 0; t < mWriterThreads; t++) mWriters.emplace_back([this] { WriterLoop(); });
  }
  const size_t rows = rows_ext - mStartExt - mEndExt;
  hipStream_t st = CuDevice::Instantiate().Stream();

  // host rows -> pinned staging buffer k (waiting only for the copy of two utterances ago) -> device
  const int k = (int)(mUtts & 1);
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

  const CuMatrix<BaseFloat>* fea = &mRaw;
  if (mTransform) {
    mTransform->Propagate(mRaw, mFea);
    fea = &mFea;
  }

  const size_t utt = mResults.size();
  mResults.emplace_back();
  Result& res = mResults.back();
  res.logical = logical;
  res.rows = rows;
  res.cols = mC;
  res.sample_period = sample_period;
  res.remaining = rows * mC;
  if (!mFile) res.words.reset(new uint32_t[rows * mC]);
  mUtts++;
  mFrames += rows;

  if (!mPacked) {  // the reference's route: the whole extended utterance through the network, trimmed by the emit
    Slot& s = mSlot[mCur];
    s.pieces.push_back(Piece{utt, 0, 0, rows});
    RunNetwork(*fea, mStartExt, rows);
    return;
  }
  mPack.Init(mPackRows, mNetIn);
  for (size_t done = 0; done < rows;) {
    const size_t take = std::min(rows - done, mPackRows - mFill);
    mPack.CopyRows(take, mStartExt + done, *fea, mFill);
    mSlot[mCur].pieces.push_back(Piece{utt, done, mFill, take});
    mFill += take;
    done += take;
    if (mFill == mPackRows) FlushPack();
  }
}

void CuFeaCat::FlushPack() {
  if (!mFill) return;
  const CuMatrix<BaseFloat>* in = &mPack;
  if (mFill < mPackRows) {
    CuMatrix<BaseFloat>::MakeView(mView, mPack.pCUData(), mFill, mPack.Cols(), mPack.Stride());
    in = &mView;
  }
  const size_t rows = mFill;
  mFill = 0;
  RunNetwork(*in, 0, rows);
}

void CuFeaCat::RunNetwork(const CuMatrix<BaseFloat>& in, size_t src_row, size_t rows) {
  Slot& s = mSlot[mCur];
  if (s.in_flight) Error("CuFeaCat: the slot of this pack has not been drained");  // (it was, a pack ago)
  WaitWritten(s);  // the writers of the pack that used this slot kSlots packs ago
  Reserve(s, (mPacked ? mPackRows : rows) * mC);
  hipStream_t st = CuDevice::Instantiate().Stream();

  const int n = mNet->Layers();
  const int upto = mSoftmaxTop ? n - 1 : n;
  const CuMatrix<BaseFloat>* y = &in;
  if (n) {
    if (in.Cols() != mNet->GetNInputs()) Error("CuFeaCat: the network's input dimension does not match");
    mNet->Layer(0).SetInput(in);
    for (int i = 0; i < upto; i++) mNet->Layer(i).Propagate();
    if (upto > 0) y = &mNet->Layer(upto - 1).GetOutput();
  }
  if (y->Cols() != mC) Error("CuFeaCat: unexpected output dimension");
  const int seg_src = (int)src_row, seg_dst = 0, seg_rows = (int)rows;
  if (mSoftmaxTop)
    TNET_SAFE_CALL(tnet_softmax_emit(y->pCUData(), y->Dim(), &seg_src, &seg_dst, &seg_rows, 1, mMode, mSwap ? 1 : 0,
                                     s.dense, st));
  else
    TNET_SAFE_CALL(tnet_feacat_emit(y->pCUData(), y->Dim(), &seg_src, &seg_dst, &seg_rows, 1, mMode, mSwap ? 1 : 0,
                                    s.dense, st));
  // the copy stream takes the pack once the emit has written it; the library stream goes on with the next pack
  TNET_HIP_CALL(hipEventRecord(s.emitted, st));
  TNET_HIP_CALL(hipStreamWaitEvent(mCopyStream, s.emitted, 0));
  TNET_HIP_CALL(hipMemcpyAsync(s.pinned, s.dense, rows * mC * sizeof(uint32_t), hipMemcpyDeviceToHost, mCopyStream));
  TNET_HIP_CALL(hipEventRecord(s.drained, mCopyStream));
  s.in_flight = true;
  mPacks++;
  // while this pack computes and copies, cut the previous one into its utterances
  Slot& prev = mSlot[(mCur + kSlots - 1) % kSlots];
  if (prev.in_flight) Drain(prev);
  mCur = (mCur + 1) % kSlots;
}

void CuFeaCat::Drain(Slot& s) {
  TNET_HIP_CALL(hipEventSynchronize(s.drained));  // the one wait of a pack
  s.in_flight = false;
  std::vector<Job> jobs;
  for (const Piece& p : s.pieces) {
    Result& r = mResults[p.utt];
    const size_t n = p.rows * mC;
    const uint32_t* src = s.pinned + p.slot_row * mC;
    if (!mFile) {
      std::memcpy(r.words.get() + p.utt_row * mC, src, n * sizeof(uint32_t));
      continue;
    }
    if (!r.opened) OpenFile(r);
    if (r.fd >= 0) jobs.push_back(Job{&r, &s, src, n, p.utt_row * mC});
  }
  s.pieces.clear();
  if (jobs.empty()) return;
  {
    std::lock_guard<std::mutex> lk(mMu);
    s.pending += (int)jobs.size();
    for (const Job& j : jobs) mJobs.push_back(j);
  }
  mCv.notify_all();
}

void CuFeaCat::WriteError(const std::string& msg) {
  std::lock_guard<std::mutex> lk(mMu);
  if (mWriteError.empty()) mWriteError = msg;
}

void CuFeaCat::OpenFile(Result& r) {
  r.opened = true;
  r.path = tnetio::MakeHtkFileName(r.logical, mHasDir ? mDir.c_str() : nullptr, mExt.c_str());
  r.fd = open(r.path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (r.fd < 0) {
    WriteError("CuFeaCat: " + r.logical + ": Cannot open output feature file: '" + r.path + "': " + strerror(errno));
    return;
  }
  unsigned char head[12];
  tnetio::EncodeHtkHeader(head, r.rows, r.cols, r.sample_period, tnetio::kParmUser, mSwap);
  if (pwrite(r.fd, head, 12, 0) != 12) r.write_failed = true;
}

void CuFeaCat::WaitWritten(Slot& s) {
  std::unique_lock<std::mutex> lk(mMu);
  mCv.wait(lk, [&s] { return s.pending == 0; });
}

void CuFeaCat::WriterLoop() {
  for (;;) {
    Job j;
    {
      std::unique_lock<std::mutex> lk(mMu);
      mCv.wait(lk, [this] { return mStop || !mJobs.empty(); });
      if (mJobs.empty()) return;
      j = mJobs.front();
      mJobs.pop_front();
    }
    const char* p = (const char*)j.src;
    size_t left = j.words * sizeof(uint32_t);
    off_t at = (off_t)(12 + j.word_off * sizeof(uint32_t));
    while (left) {
      const ssize_t n = pwrite(j.r->fd, p, left, at);
      if (n < 0 && errno == EINTR) continue;
      if (n <= 0) {
        j.r->write_failed = true;
        break;
      }
      p += n;
      at += n;
      left -= (size_t)n;
    }
    if (j.r->remaining.fetch_sub(j.words) == j.words) {  // the utterance's last piece: this thread closes the file
      bool bad = j.r->write_failed;
      if (close(j.r->fd) != 0) bad = true;
      j.r->fd = -1;
      if (bad) {
        remove(j.r->path.c_str());
        WriteError("CuFeaCat: " + j.r->logical + ": Cannot write to output feature file: '" + j.r->path + "'");
      }
    }
    {
      std::lock_guard<std::mutex> lk(mMu);
      j.slot->pending--;
    }
    mCv.notify_all();
  }
}

void CuFeaCat::StopWriters() {
  {
    std::lock_guard<std::mutex> lk(mMu);
    mStop = true;
  }
  mCv.notify_all();
  for (std::thread& t : mWriters) t.join();
  mWriters.clear();
}

long CuFeaCat::AddReader(tnetio::FeatureReader& reader, size_t reader_start_ext, size_t reader_end_ext,
                         long max_utts) {
  if (reader_start_ext != mStartExt || reader_end_ext != mEndExt) {
    std::ostringstream os;
    os << "CuFeaCat::AddReader: the reader carries " << reader_start_ext << "/" << reader_end_ext
       << " context rows, the pass expects " << mStartExt << "/" << mEndExt;
    Error(os.str());
  }
  const unsigned long before = mFrames;
  for (long n = 0; max_utts < 0 || n < max_utts; n++) {
    const tnetio::Utterance* u = reader.Next();
    if (!u) break;
    AddUtterance(u->feats.data(), (size_t)u->rows, (size_t)u->cols, (size_t)u->cols, u->logical, u->samplePeriod);
  }
  return (long)(mFrames - before);
}

void CuFeaCat::Finish() {
  if (mFinished) return;
  if (mPacked) FlushPack();
  for (int k = 1; k <= kSlots; k++) {  // oldest first: the slot after the current one was used longest ago
    Slot& s = mSlot[(mCur + k) % kSlots];
    if (s.in_flight) Drain(s);
  }
  for (Slot& s : mSlot) WaitWritten(s);
  if (mInFlight[0] || mInFlight[1]) {
    TNET_HIP_CALL(hipStreamSynchronize(CuDevice::Instantiate().Stream()));
    mInFlight[0] = mInFlight[1] = false;
  }
  StopWriters();
  mFinished = true;
  if (!mWriteError.empty()) Error(mWriteError);
}

const CuFeaCat::Result& CuFeaCat::Fetch(size_t i) const {
  if (!mFinished) Error("CuFeaCat::Fetch: Finish() first");
  if (mFile) Error("CuFeaCat::Fetch: the results went to files");
  if (i >= mResults.size()) Error("CuFeaCat::Fetch: no such utterance");
  return mResults[i];
}

}  // namespace TNet
