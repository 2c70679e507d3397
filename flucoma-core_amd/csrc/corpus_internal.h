// corpus_internal.h -- what the three translation units of the corpus layer share beyond api_internal.h
// (corpus_plan.hip: the planner, corpus_loop.hip: the iteration loop, api_corpus.hip: allocation and the C ABI).
#pragma once

#include "api_internal.h"

#pragma GCC visibility push(hidden)

// the work lists of the two factor updates as build_list_plan leaves them on the host (corpus_plan.hip)
struct ListSide
{
  std::vector<WaveDesc> list;
  std::vector<int> splitTab;
  int wgs = 0, ng = 0, partial = 0, maxSplit = 1, pieces = 1, statParts = 0;
  int64_t nPartials = 0;
};
struct ListPlanHost
{
  ListSide W, H;
  bool sideW = false;
};

// corpus_plan.hip
// (lists: where an equal-length shape that takes the work lists leaves them, for the upload)
void decide_update_plan(int64_t B, int64_t T, int64_t F, int64_t K, UpdatePlan& p, ListPlanHost* lists = nullptr);
void decide_list_plan(const std::vector<int>& tOf, int64_t T, int64_t F, int64_t K, UpdatePlan& p, ListPlanHost& lp);
int plain_h_update_takes(UpdateArgs a, bool wantNorm, int colInN);

#pragma GCC visibility pop
