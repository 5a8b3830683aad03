// ALE Navier-Stokes driver on the MI355X path (a test harness, like the other drivers): the fluid half of one step of the
// reference's FSI problem (feddlib/problems/specific/FSI_def.hpp:445-464, 497-503, 644-678) on a structured P2 / P1 domain,
// written against the FEDD:: operator surface:
//   Domain::buildMesh x 2 -> an analytic displacement that vanishes on the boundary -> Domain::moveMesh (both domains)
//   -> the mesh velocity w = (d_new - d_old) * (1 / dt) from two such displacements (fedd_mesh_velocity_diff)
//   -> NavierStokes(...) -> addBoundaries -> initializeProblem -> assemble (the constant matrices, on the moved mesh)
//   -> P = FE::assemblyAdditionalConvection(w), scaled by density and by -1 (FSI_def.hpp:497-503)
//   -> the fixed-point loop: calculateNonLinResidualVecWithMeshVelo("reverse", 0, u - w, P) -> setBoundariesSystem ->
//      solveAndUpdate, to "relNonLinTol"
//   -> the solution by global dof id.
// --provoke=wrongP | wrongScale | wrongDiff | newton makes the one wrong call named and reports the facade's error.
// Out of scope: TimeProblem / DAESolverInTime on a moving mesh, the FSI problem class, geometry-implicit coupling, shape
// derivatives, more than one rank.
#include <cmath>
#include <cstring>
#include <fstream>
#include <iomanip>

#include "feddlib/core/FEDDCore.hpp"
#include "feddlib/core/FE/Domain.hpp"
#include "feddlib/core/General/BCBuilder.hpp"
#include "feddlib/problems/specific/NavierStokes.hpp"
#include "feddlib/problems/abstract/NonLinearProblem.hpp"

void zeroDirichlet2D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; }
void zeroDirichlet3D(double* x, double* res, double t, const double* parameters) { res[0] = 0.; res[1] = 0.; res[2] = 0.; }
void inflowParabolic2D(double* x, double* res, double t, const double* parameters) {
    double H = parameters[1];
    res[0] = 4 * parameters[0] * x[1] * (H - x[1]) / (H * H);
    res[1] = 0.;
}
void inflowParabolic3D(double* x, double* res, double t, const double* parameters) {
    double H = parameters[1];
    res[0] = 16 * parameters[0] * x[1] * (H - x[1]) * x[2] * (H - x[2]) / (H * H * H * H);
    res[1] = 0.;
    res[2] = 0.;
}

typedef default_sc SC;
typedef default_lo LO;
typedef default_go GO;
typedef default_no NO;

using namespace FEDD;
typedef MultiVector<SC, LO, GO, NO> MV;
typedef Teuchos::RCP<Domain<SC, LO, GO, NO> > DomainPtr_Type;

// d_k(x) = a * prod_j sin(pi x_j) * cos(2.1 x_{k+1} + 0.7 k), exactly zero on the boundary of the unit square / cube
static void displacement(const std::vector<double>& xyz, int dim, double a, std::vector<double>& d) {
    const double pi = 3.141592653589793;
    d.assign(xyz.size(), 0.);
    for (size_t i = 0; i < xyz.size() / dim; ++i) {
        const double* x = &xyz[i * dim];
        bool onBoundary = false;
        double bubble = 1.;
        for (int j = 0; j < dim; ++j) {
            onBoundary = onBoundary || x[j] == 0. || x[j] == 1.;
            bubble *= std::sin(pi * x[j]);
        }
        if (onBoundary) continue;
        for (int k = 0; k < dim; ++k) d[i * dim + k] = a * bubble * std::cos(2.1 * x[(k + 1) % dim] + 0.7 * k);
    }
}

static void moveDomain(const DomainPtr_Type& domain, int dim, const std::vector<double>& dRep) {
    Teuchos::RCP<MV> rep(new MV(domain->getMapVecFieldRepeated())), uni(new MV(domain->getMapVecFieldUnique()));
    rep->raw(0) = dRep;
    const auto& uniOfRep = domain->uniqueLocalOfRepeated();
    for (size_t i = 0; i < uniOfRep.size(); ++i)
        for (int k = 0; k < dim; ++k) uni->raw(0)[i * dim + k] = dRep[(size_t)uniOfRep[i] * dim + k];
    domain->moveMesh(uni, rep);
}

int main(int argc, char* argv[]) {
    std::string xmlProblemFile = "parametersProblem.xml", xmlPrecFile = "parametersPrec.xml", xmlSolverFile = "parametersSolver.xml";
    std::string outFile = "solutionAleNavierStokes.txt", provoke;
    for (int i = 1; i < argc; ++i) {
        std::string a(argv[i]);
        auto val = [&](const char* key, std::string& dst) {
            const std::string k = std::string("--") + key + "=";
            if (a.compare(0, k.size(), k) == 0) { dst = a.substr(k.size()); return true; }
            return false;
        };
        if (val("problemfile", xmlProblemFile) || val("precfile", xmlPrecFile) || val("solverfile", xmlSolverFile) || val("out", outFile) ||
            val("provoke", provoke)) continue;
        std::cerr << "unknown option " << a << std::endl;
        return 2;
    }
    try {
        Teuchos::RCP<const Teuchos::Comm<int> > comm = Teuchos::rcp(new Teuchos::Comm<int>(0, 1));
        ParameterListPtr_Type parameterListProblem = Teuchos::getParametersFromXmlFile(xmlProblemFile);
        ParameterListPtr_Type parameterListPrec = Teuchos::getParametersFromXmlFile(xmlPrecFile);
        ParameterListPtr_Type parameterListSolver = Teuchos::getParametersFromXmlFile(xmlSolverFile);
        ParameterListPtr_Type parameterListAll(new Teuchos::ParameterList(*parameterListProblem));
        parameterListAll->setParameters(*parameterListPrec);
        parameterListAll->setParameters(*parameterListSolver);
        auto& par = parameterListProblem->sublist("Parameter");
        const int dim = par.get("Dimension", 2), m = par.get("H/h", 4);
        const std::string discVelocity = par.get("Discretization Velocity", "P2"), discPressure = par.get("Discretization Pressure", "P1");
        const double density = par.get("Density", 1.), aOld = par.get("Mesh Amplitude Old", 0.), aNew = par.get("Mesh Amplitude New", 0.);
        const double dt = par.get("Mesh Time Step", 1.), tol = par.get("relNonLinTol", 1.0e-6);
        const int maxNonLinIts = par.get("MaxNonLinIts", 10);
        TEUCHOS_TEST_FOR_EXCEPTION(par.get("Mesh Type", "structured") != "structured", std::logic_error, "this driver builds structured meshes");
        TEUCHOS_TEST_FOR_EXCEPTION(discVelocity != "P2" || discPressure != "P1", std::logic_error, "this driver builds P2 / P1");

        // ---- 1. the two domains ----
        std::vector<double> x0(dim, 0.0);
        DomainPtr_Type domainPressure, domainVelocity;
        if (dim == 2) {
            domainPressure.reset(new Domain<SC, LO, GO, NO>(x0, 1., 1., comm));
            domainVelocity.reset(new Domain<SC, LO, GO, NO>(x0, 1., 1., comm));
        } else {
            domainPressure.reset(new Domain<SC, LO, GO, NO>(x0, 1., 1., 1., comm));
            domainVelocity.reset(new Domain<SC, LO, GO, NO>(x0, 1., 1., 1., comm));
        }
        domainPressure->buildMesh(1, "Square", dim, discPressure, 1, m, 0);
        domainVelocity->buildMesh(1, "Square", dim, discVelocity, 1, m, 0);

        // ---- 2. two displacements of the reference points, the move by the new one, the mesh velocity from both ----
        std::vector<double> dOldV, dNewV, dNewP;
        displacement(domainVelocity->xyzRepeated(), dim, aOld, dOldV);
        displacement(domainVelocity->xyzRepeated(), dim, aNew, dNewV);
        displacement(domainPressure->xyzRepeated(), dim, aNew, dNewP);
        moveDomain(domainVelocity, dim, dNewV);
        moveDomain(domainPressure, dim, dNewP);
        fedd_ctx* ctx = domainVelocity->device()->ctx;
        feddCheck(fedd_mesh_velocity_diff(ctx, dNewV.data(), dOldV.data(), dt), "fedd_mesh_velocity_diff");
        Teuchos::RCP<MV> w(new MV(domainVelocity->getMapVecFieldRepeated()));
        feddCheck(fedd_mesh_velocity_get(ctx, w->raw(0).data()), "fedd_mesh_velocity_get");
        double minDetRatio = 0.;
        feddCheck(fedd_mesh_move_info(ctx, nullptr, nullptr, &minDetRatio), "fedd_mesh_move_info");

        // ---- 3. the problem and its constant matrices on the moved mesh ----
        std::vector<double> parameter_vec(1, par.get("MaxVelocity", 1.));
        parameter_vec.push_back(1.);
        Teuchos::RCP<BCBuilder<SC, LO, GO, NO> > bcFactory(new BCBuilder<SC, LO, GO, NO>());
        bcFactory->addBC(dim == 2 ? zeroDirichlet2D : zeroDirichlet3D, 1, 0, domainVelocity, "Dirichlet", dim);
        bcFactory->addBC(dim == 2 ? inflowParabolic2D : inflowParabolic3D, 2, 0, domainVelocity, "Dirichlet", dim, parameter_vec);
        NavierStokes<SC, LO, GO, NO> navierStokes(domainVelocity, discVelocity, domainPressure, discPressure, parameterListAll);
        navierStokes.addBoundaries(bcFactory);
        navierStokes.initializeProblem();
        navierStokes.assemble();
        navierStokes.setBoundariesRHS();

        // ---- 4. P = -density P(w) (FSI_def.hpp:497-503) ----
        typedef Matrix<SC, LO, GO, NO> Matrix_Type;
        auto mapV = domainVelocity->getMapVecFieldUnique();
        Teuchos::RCP<Matrix_Type> P(new Matrix_Type(mapV, dim * domainVelocity->getApproxEntriesPerRow()));
        navierStokes.getFEFactory()->assemblyAdditionalConvection(dim, discVelocity, P, w, true);
        P->resumeFill();
        P->scale(density);
        if (provoke != "wrongScale") P->scale(-1.0);
        P->fillComplete(mapV, mapV);
        if (provoke == "wrongP") {      // another P(w) is built after this one: P is no longer the last
            Teuchos::RCP<Matrix_Type> P2(new Matrix_Type(mapV, dim * domainVelocity->getApproxEntriesPerRow()));
            navierStokes.getFEFactory()->assemblyAdditionalConvection(dim, discVelocity, P2, w, true);
        }

        // ---- 5. the fixed-point loop ----
        Teuchos::RCP<MV> uMinusW(new MV(domainVelocity->getMapVecFieldRepeated()));
        const auto& uniOfRep = domainVelocity->uniqueLocalOfRepeated();
        double residual0 = 1., criterionValue = 1.;
        int nlIts = 0;
        double gmresIts = 0.;
        while (nlIts < maxNonLinIts) {
            const auto& u = navierStokes.getSolution()->getBlock(0)->raw();
            for (size_t i = 0; i < uniOfRep.size(); ++i)
                for (int k = 0; k < dim; ++k) {
                    const size_t r = (size_t)uniOfRep[i] * dim + k;
                    uMinusW->raw(0)[r] = u[i * dim + k] - w->raw(0)[r];
                }
            if (provoke == "wrongDiff") uMinusW->raw(0)[uMinusW->raw(0).size() / 2] += 1.0e-3;
            if (provoke == "newton") navierStokes.reAssembleFSI("Newton", uMinusW, P);
            navierStokes.calculateNonLinResidualVecWithMeshVelo("reverse", 0., uMinusW, P);
            navierStokes.setBoundariesSystem();
            const double residual = navierStokes.calculateResidualNorm();
            if (nlIts == 0) residual0 = residual;
            criterionValue = residual / residual0;
            std::cout << "### ALE fixed point iteration : " << nlIts << "  relative nonlinear residual : " << criterionValue << std::endl;
            if (criterionValue < tol) break;
            gmresIts += navierStokes.solveAndUpdate("Residual", criterionValue);
            nlIts++;
        }
        std::cout << "nonlinear iterations " << nlIts << " residual " << std::setprecision(17) << criterionValue << " gmres "
                  << gmresIts / std::max(nlIts, 1) << " min_det_ratio " << minDetRatio << std::endl;
        TEUCHOS_TEST_FOR_EXCEPTION(criterionValue >= tol, std::runtime_error, "the fixed-point loop did not reach relNonLinTol");

        // ---- 6. the solution by global dof id ----
        auto solV = navierStokes.getSolution()->getBlock(0);
        auto solP = navierStokes.getSolution()->getBlock(1);
        std::ofstream out(outFile);
        out << std::setprecision(17);
        auto mapVn = domainVelocity->getMapUnique();
        auto mapPn = domainPressure->getMapUnique();
        for (size_t i = 0; i < solV->getLocalLength(); ++i)
            out << (size_t)mapVn->getGlobalElement((LO)(i / dim)) * dim + i % dim << " " << solV->getData(0)[i] << "\n";
        const size_t off = solV->getLocalLength();
        for (size_t i = 0; i < solP->getLocalLength(); ++i) out << off + (size_t)mapPn->getGlobalElement((LO)i) << " " << solP->getData(0)[i] << "\n";
    } catch (const std::exception& e) {
        std::cerr << "exception: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
