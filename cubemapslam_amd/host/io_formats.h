// io_formats.h -- the reference's file formats around the hot path, plain C++ (no OpenCV, no GPU):
//   settings YAML          cv::FileStorage keys read at src/System.cpp:63-91 and src/Tracking.cpp:61-93 (Config/*.yaml)
//   image lists            Examples/cubemap_lafida.cpp:91-107 ("<timestamp> <path>" per line, directory stripped) and
//                          Examples/cubemap_fangshan.cpp:93-101 ("<timestamp>_<suffix>" file names, one per line)
//   tracking-time summary  Examples/cubemap_lafida.cpp:160-179
//   vocabulary text        DBoW2 TemplatedVocabulary.h:1338-1449 (loadFromTextFile / saveToTextFile: ORBvoc.txt)
// (the TUM key-frame trajectory writer, src/System.cpp:238-268, lives in System::SaveKeyFrameTrajectoryTUM.)
#ifndef CUBEMAPSLAM_IO_FORMATS_H
#define CUBEMAPSLAM_IO_FORMATS_H
#include <map>
#include <string>
#include <vector>
#include "cubemapslam_hip.h"

namespace CubemapSLAM {

// The YAML subset cv::FileStorage files of the reference use: "%YAML:1.0" header, comments, flat "Key.sub: scalar" lines.
class Settings {
 public:
  bool Load(const std::string& path);                 // false when the file cannot be opened
  bool LoadFromString(const std::string& text);
  bool Has(const std::string& key) const { return values_.count(key) != 0; }
  double Real(const std::string& key) const;          // cv::FileNode -> double; a missing key reads as 0 like an empty FileNode
  int Int(const std::string& key) const;              // cv::FileNode -> int (rounds a real like cvRound)
  std::string String(const std::string& key) const;
  // System.cpp:63-89: polynomial arrays zero padded to 5 / 12 entries, Camera.{Iw,Ih,c,d,e,u0,v0,fov}, CubeFace.w
  cms_camera Camera() const;
  // Tracking.cpp:88-96
  cms_orb_params Orb() const;
  float Fps() const;                                  // Camera.fps, 30 when 0 or absent (Tracking.cpp:66-68)
  int WithFisheyeMask() const { return Int("Camera.withFisheyeMask"); }
  bool RGB() const { return Int("Camera.RGB") != 0; }

 private:
  std::map<std::string, std::string> values_;
};

struct ImageList { std::vector<std::string> names; std::vector<double> timestamps; };
ImageList LoadImageListLafida(const std::string& path);     // cubemap_lafida.cpp:91-107
ImageList LoadImageListFangshan(const std::string& path);   // cubemap_fangshan.cpp:93-101

// cubemap_lafida.cpp:160-179: sorts the times, median = v[n/2], mean = float sum / n; writes the perf file and returns the text
// the reference prints to stdout.  vTimesTrack is sorted in place like the reference does.
std::string WriteTrackingSummary(const std::string& perfSavingPath, std::vector<float>& vTimesTrack, int frame_counter);

// The vocabulary tree as the text format holds it (TemplatedVocabulary.h:1338-1449): a header line "k L  scoring weighting", then one line per node
// from node 1 on, "parent leaf d0 .. d31  weight".  Node 0 is the root; arrays have one entry per node (the root's are zero).
struct VocabularyText {
  int k = 0, L = 0, scoring = 0, weighting = 0;
  std::vector<int> parent;
  std::vector<uint8_t> is_leaf;
  std::vector<uint8_t> desc;        // nodes x 32
  std::vector<double> weight;
  int nodes() const { return (int)parent.size(); }
};
// The parser reads what loadFromTextFile reads, with one known difference: empty lines are skipped (the reference turns a trailing empty line
// into an extra child of the root with an uninitialised descriptor).  A header outside the reference's ranges (:1359) or a node line that ends
// early is refused with the reason in *why; the tree's shape is checked by cms_vocab_relayout (csrc/cms_vocab_core.h).
bool ParseVocabularyText(const std::string& text, VocabularyText* out, std::string* why);
bool LoadVocabularyText(const std::string& path, VocabularyText* out, std::string* why);
// saveToTextFile's bytes (:1429-1449): "<k> <L>  <scoring> <weighting>\n", then "<parent> <0|1> <32 bytes, each followed by a space> <weight>\n"
// with the weight in the stream's default format (6 significant digits)
std::string FormatVocabularyText(const VocabularyText& v);

}  // namespace CubemapSLAM
#endif
