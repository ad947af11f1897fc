// The one switch from a runtime game id (AZMI_GAME_*) to the game type the kernels are instantiated with.
#pragma once
#include "../../include/azmi.h"
#include "dev_games.h"
#include "dev_stargambit.h"

namespace azmi {

// small(Connect4{}) for the lane-group engine, big(GM{}) for the games that run one wavefront per tree; the callee names its game
// with `using GM = decltype(tag)`.  Callers validate the id when their object is created; here any other id runs as OpenTafl, as it
// does in the MCTS object (search_batch.hip keeps a switch of its own, whose last arm is StarGambit).
template <class Small, class Big>
void for_game(int game, Small&& small, Big&& big) {
  switch (game) {
    case AZMI_GAME_CONNECT4: small(Connect4{}); break;
    case AZMI_GAME_TAWLBWRDD: big(Tawlbwrdd{}); break;
    case AZMI_GAME_BRANDUBH: big(Brandubh{}); break;
    case AZMI_GAME_STARGAMBIT: big(StarGambit{}); break;
    default: big(OpenTafl{}); break;
  }
}

}  // namespace azmi
