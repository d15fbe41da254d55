// cufeacat.h -- CuFeaCat: the TFeaCatCu loop (src/TFeaCatCu.cc:215-270) as a library object.
//
// TFeaCatCu turns a trained network into feature files: per utterance it uploads the (frame-extended) features,
// propagates them through the feature transform and the network, trims the context rows, copies the output back,
// applies GMMBYPASS / LOGPOSTERIOR element by element on the host and writes an HTK file, swapping every word on
// the same thread.  Here:
//
//   per utterance   pinned staging -> device, the borrowed transform (always per utterance: <expand> splices
//                   neighbouring rows), then the rows BETWEEN the context rows appended to a packing buffer
//   per pack        the network once over pack_rows rows of back-to-back utterances (an utterance may straddle two
//                   packs) -- the bunch shape the GEMMs were tuned for instead of whatever an utterance happens to
//                   have, and no network work on rows that are thrown away; then ONE emit kernel (tnet_softmax_emit
//                   when the last component is <softmax>, tnet_feacat_emit otherwise): mode, byte order and the
//                   dense file layout on the device
//   sink            one async device -> pinned copy per pack on a copy stream into a ring of three slots: pack n + 1
//                   computes while pack n copies and pack n - 1 is written.  One event wait per pack, nothing
//                   synchronises per utterance.  A drained pack is cut into per-utterance pieces; a small writer pool
//                   pwrites each piece from the pinned slot straight to its place in the utterance's file (opened, and
//                   its 12-byte header written, when the first piece arrives; an utterance that straddles packs is
//                   written piece by piece), or, without SetOutput, the pieces are copied into arrays kept for Fetch.
//
// Packing is safe exactly when no component mixes rows (CuComponent::IsRowWise for every component): row i of the
// output then depends on row i of the input alone, so which other rows share the GEMM does not matter, and the
// context rows -- which exist only to feed the transform's <expand> -- can go before the network.  Any other network
// (<expand>, <recurrent>, <blockarray>, ... inside) takes the reference's route: one utterance a pass, all rows through
// the network, the context rows dropped by the emit's segment table.  Same kernels, same sink.
//
// Errors are raised before the pass's first launch where they can be known then (dimension mismatch between the
// transform and the network, more than 8191 output columns: the HTK sample size is an int16 and the reference
// overflows silently) or at the utterance that shows them (rows <= start_ext + end_ext, feature dimension), naming it.
// A file that cannot be created is reported by Finish, naming the file; the other utterances are written in full.
// A non-finite input feature is data (the reference only warns).
#pragma once

#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "cunetwork.h"

namespace tnetio {
class FeatureReader;
}

namespace TNet {

class CuFeaCat {
 public:
  static constexpr size_t kDefaultPackRows = 4096;  // profiles/feacat.json: the sweep over {1024 .. 8192}

  /// net, transform: borrowed; transform may be nullptr or empty.  mode: TNET_FEACAT_* bits.  pack_rows 0: default.
  /// pack = false: one utterance a pass whatever the network (the reference's route; for comparisons).
  CuFeaCat(CuNetwork* net, CuNetwork* transform, size_t start_ext, size_t end_ext, int mode, size_t pack_rows,
           bool pack = true);
  ~CuFeaCat();
  CuFeaCat(const CuFeaCat&) = delete;
  CuFeaCat& operator=(const CuFeaCat&) = delete;

  /// File sink: TARGETPARAMDIR / basename(logical) . TARGETPARAMEXT by MakeHtkFileName; swap: big-endian files.
  /// Without it the results are kept in memory (host byte order unless `swap`).  Only before the first utterance.
  void SetOutput(const char* dir, const char* ext, bool swap, int writer_threads = 2);
  /// memory sink: the byte order of the kept words (default: host order)
  void SetSwap(bool swap);

  void AddUtterance(const float* feats, size_t rows_ext, size_t cols, size_t ld, const std::string& logical,
                    int sample_period);
  long AddReader(tnetio::FeatureReader& reader, size_t reader_start_ext, size_t reader_end_ext, long max_utts);
  /// the last (partial) pack, the drain, the writers; throws the first writer error
  void Finish();

  struct Result {
    std::string logical;
    size_t rows = 0, cols = 0;
    int sample_period = 0;
    std::unique_ptr<uint32_t[]> words;  // memory sink: rows * cols words, as emitted
    // file sink: the file is opened (and its header written) when the utterance's first piece drains; the writers
    // pwrite the pieces straight from the pinned ring and the one that writes the last word closes it
    std::string path;
    int fd = -1;
    bool opened = false;
    std::atomic<size_t> remaining{0};  // words not yet written
    std::atomic<bool> write_failed{false};
  };
  /// memory sink, after Finish: utterances in the order they were added
  size_t Results() const { return mFile ? 0 : mResults.size(); }
  const Result& Fetch(size_t i) const;

  unsigned long Frames() const { return mFrames; }
  unsigned long Utterances() const { return mUtts; }
  unsigned long Packs() const { return mPacks; }
  bool Packed() const { return mPacked; }
  size_t PackRows() const { return mPackRows; }
  size_t Cols() const { return mC; }

 private:
  struct Piece {  // rows of one utterance inside a slot's dense buffer
    size_t utt, utt_row, slot_row, rows;
  };
  struct Slot {
    uint32_t* dense = nullptr;   // device, cap words
    uint32_t* pinned = nullptr;  // host
    size_t cap = 0;
    hipEvent_t emitted = nullptr, drained = nullptr;
    bool in_flight = false;
    int pending = 0;  // write jobs reading `pinned` (under mMu): the slot is reused when they are done
    std::vector<Piece> pieces;
  };
  struct Job {  // `words` words at `src` (pinned) -> word `word_off` of r's body
    Result* r;
    Slot* slot;
    const uint32_t* src;
    size_t words, word_off;
  };
  static constexpr int kSlots = 3;
  void CheckDims(size_t cols);
  void Reserve(Slot& s, size_t words);
  void RunNetwork(const CuMatrix<BaseFloat>& in, size_t src_row, size_t rows);  // -> emit -> copy, current slot
  void FlushPack();
  void Drain(Slot& s);
  void WaitWritten(Slot& s);
  void OpenFile(Result& r);
  void WriteError(const std::string& msg);
  void WriterLoop();
  void StopWriters();

  CuNetwork* mNet;
  CuNetwork* mTransform;
  size_t mStartExt, mEndExt;
  int mMode;
  size_t mPackRows;
  bool mPacked = false, mSoftmaxTop = false;
  size_t mC = 0, mNetIn = 0;
  bool mSwap = false, mFile = false, mHasDir = false, mStarted = false, mFinished = false;
  std::string mDir, mExt;
  int mWriterThreads = 2;

  hipStream_t mCopyStream = nullptr;
  // pinned upload staging, as CuNormAccumulator: utterance k through buffer k % 2
  float* mPinned[2] = {nullptr, nullptr};
  size_t mPinnedFloats[2] = {0, 0};
  hipEvent_t mCopied[2] = {nullptr, nullptr};
  bool mInFlight[2] = {false, false};
  CuMatrix<BaseFloat> mRaw, mFea, mPack, mView;
  size_t mFill = 0;  // rows in mPack
  Slot mSlot[kSlots];
  int mCur = 0;

  std::deque<Result> mResults;  // every utterance in order (a deque: the writers hold pointers)
  unsigned long mFrames = 0, mUtts = 0, mPacks = 0;

  // writer pool
  std::vector<std::thread> mWriters;
  std::mutex mMu;
  std::condition_variable mCv;
  std::deque<Job> mJobs;
  bool mStop = false;
  std::string mWriteError;
};

}  // namespace TNet
