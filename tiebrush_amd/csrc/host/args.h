// args.h — tiny option parser with the option-string grammar the reference hands to gclib's GArgs
// ("long;long;...;SMh" + "o:" for short options that take a value), enough to keep the tiebrush /
// tiecov command lines (tiebrush.cpp:605, tiecov.cpp:533) working verbatim.
#pragma once
#include <map>
#include <string>
#include <vector>

class Args {
 public:
  Args(int argc, char** argv, const char* fmt);
  // value of a short (single char) or long option; nullptr when absent; "" for flags that are present
  const char* getOpt(const char* name) const;
  const char* getOpt(char c) const {
    char b[2] = {c, 0};
    return getOpt(b);
  }
  int startNonOpt() {
    pos_ = 0;
    return (int)nonopt_.size();
  }
  const char* nextNonOpt() { return pos_ < nonopt_.size() ? nonopt_[pos_++].c_str() : nullptr; }
  const std::string& error() const { return err_; }
  void printCmdLine(FILE* f) const;

 private:
  std::map<std::string, std::string> opts_;
  std::vector<std::string> nonopt_, argv_;
  size_t pos_ = 0;
  std::string err_;
};

// How often a repeatable-looking option is given on a command line: Args keeps the last value of a repeated option, so a tool that takes
// one value only (tiecov / tiebrush -r REGION: one region per run) counts the occurrences itself.  long_name / short_name: the option
// counted, which takes a value; value_longs (NULL-terminated) / value_shorts: the tool's other options that take a value in the next word
// (or, short ones, in the rest of their word), whose values are not looked at.
int count_value_option(int argc, char** argv, const char* long_name, char short_name, const char* const* value_longs, const char* value_shorts);
